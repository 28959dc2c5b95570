// vpk_lines.hip -- line geometry outside the EM, batched: calc_lsim for many images in one launch
// (vpk_line_similarity_batch) and line_rating_knn + lines_angles + line_length without a distance matrix
// (vpk_line_rating_batch; see include/vpk.h).  The arithmetic and both kernel bodies are line_device.hpp's, which the EM
// workgroup uses too.  Compiled with -ffp-contract=off like the EM unit.
#include "line_device.hpp"
#include "batch_args.hpp"
#include "vpk_internal.hpp"

#include <vector>

using namespace vpk;

namespace {

constexpr int LINES_THREADS = 256;                     // four waves: four column chunks of a row block / 16 rated rows
constexpr size_t SIM_LDS_BYTES = (size_t)(LINES_THREADS / WAVE) * LS_WAVE_DOUBLES * sizeof(double);
constexpr size_t RATING_KS_BYTES = (size_t)(LINES_THREADS / ROWG) * LR_KS * sizeof(double);
constexpr int RATING_LDS_LINES = 1536;                 // 48 KiB of lp at most: with the scratch inside the 64 KiB every launch may ask for

// the block index is image-major: blocks_per_image blocks for every image, those past an image's size return at once
__global__ __launch_bounds__(LINES_THREADS) void line_similarity_kernel(LineBatchArgs a, int blocks_per_image) {
    line_similarity_rowblock(a, block_id() / blocks_per_image, block_id() % blocks_per_image);
}
__global__ __launch_bounds__(LINES_THREADS) void line_rating_kernel(LineBatchArgs a, int blocks_per_image) {
    line_rating_block(a, block_id() / blocks_per_image, block_id() % blocks_per_image);
}

constexpr long long LINES_NMAX = 0x7fffffffLL / 4;      // the kernels index an image's lp with ints

}  // namespace

extern "C" {

int vpk_line_similarity_batch(vpk_handle* h, int batch, const int64_t* offsets, const double* lp, double sigma,
                              const int64_t* mat_offsets, double* lsim_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0 || !(sigma > 0)) return vpk_fail(h, VPK_ERR_ARG, "vpk_line_similarity_batch: bad argument");
    if (batch == 0) return VPK_OK;
    if (!offsets || !mat_offsets) return vpk_fail(h, VPK_ERR_ARG, "vpk_line_similarity_batch: null offsets");
    long long nmax;
    if (batch_offsets(batch, offsets, &nmax, LINES_NMAX)) return vpk_fail(h, VPK_ERR_ARG, "vpk_line_similarity_batch: offsets must not decrease");
    if (batch_slots(batch, offsets, mat_offsets))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_line_similarity_batch: mat_offsets leave image b less than N_b^2 elements");
    if (nmax == 0) return VPK_OK;
    if (!lp || !lsim_out) return vpk_fail(h, VPK_ERR_ARG, "vpk_line_similarity_batch: null buffer");
    const long long bpi = (nmax + LS_RB - 1) / LS_RB;
    if (bpi * batch > 0x7fffffffLL) return vpk_fail(h, VPK_ERR_ARG, "vpk_line_similarity_batch: batch x rows too large for one launch");
    VPK_HIP(h, hipSetDevice(h->device));
    std::vector<int64_t> hdr(2 * ((size_t)batch + 1));
    for (int b = 0; b <= batch; ++b) { hdr[b] = offsets[b]; hdr[(size_t)batch + 1 + b] = mat_offsets[b]; }
    const int rc = vpk_stage_upload(h, h->lines_hdr, hdr.data(), hdr.size() * sizeof(int64_t), "vpk_line_similarity_batch: header");
    if (rc) return rc;
    LineBatchArgs a = {};
    a.offsets = (cglp)h->lines_hdr.dev;
    a.mat_offsets = a.offsets + batch + 1;
    a.lp = (cgdp)lp;
    a.sigma = sigma;
    a.lsim = (gdp)lsim_out;
    hipLaunchKernelGGL(line_similarity_kernel, dim3((unsigned)(bpi * batch)), dim3(LINES_THREADS), SIM_LDS_BYTES, h->stream, a,
                       (int)bpi);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

int vpk_line_rating_batch(vpk_handle* h, int batch, const int64_t* offsets, const double* lp, int k1, int k2, double sigma,
                          double* lscore_out, double* langle_out, double* llen_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0 || !(sigma > 0) || k1 < 1 || k1 > LR_K || k2 < 1 || k2 > k1)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_line_rating_batch: bad argument (sigma > 0, 1 <= k2 <= k1 <= 16)");
    if (batch == 0) return VPK_OK;
    if (!offsets) return vpk_fail(h, VPK_ERR_ARG, "vpk_line_rating_batch: null offsets");
    long long nmax;
    if (batch_offsets(batch, offsets, &nmax, LINES_NMAX)) return vpk_fail(h, VPK_ERR_ARG, "vpk_line_rating_batch: offsets must not decrease");
    if (nmax == 0 || (!lscore_out && !langle_out && !llen_out)) return VPK_OK;
    if (!lp) return vpk_fail(h, VPK_ERR_ARG, "vpk_line_rating_batch: null buffer");
    constexpr int rpb = LINES_THREADS / ROWG;
    const long long bpi = (nmax + rpb - 1) / rpb;
    if (bpi * batch > 0x7fffffffLL) return vpk_fail(h, VPK_ERR_ARG, "vpk_line_rating_batch: batch x rows too large for one launch");
    VPK_HIP(h, hipSetDevice(h->device));
    const int rc = vpk_stage_upload(h, h->lines_hdr, offsets, ((size_t)batch + 1) * sizeof(int64_t), "vpk_line_rating_batch: header");
    if (rc) return rc;
    // LDS for the largest image that is staged (the scores alone read other lines)
    long long staged = 0;
    if (lscore_out)
        for (int b = 0; b < batch; ++b) {
            const long long n = offsets[b + 1] - offsets[b];
            if (n <= RATING_LDS_LINES && n > staged) staged = n;
        }
    LineBatchArgs a = {};
    a.offsets = (cglp)h->lines_hdr.dev;
    a.lp = (cgdp)lp;
    a.sigma = sigma;
    a.k1 = k1; a.k2 = k2;
    a.lscore = (gdp)lscore_out; a.langle = (gdp)langle_out; a.llen = (gdp)llen_out;
    a.lds_lines = lscore_out ? RATING_LDS_LINES : 0;
    const size_t lds = RATING_KS_BYTES + (size_t)staged * 4 * sizeof(double);
    hipLaunchKernelGGL(line_rating_kernel, dim3((unsigned)(bpi * batch)), dim3(LINES_THREADS), lds, h->stream, a, (int)bpi);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // extern "C"
