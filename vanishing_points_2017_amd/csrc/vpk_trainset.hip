// vpk_trainset.hip -- batches of a device-resident training set (vpk_trainset_batch) and the integer sum behind its mean
// image (vpk_trainset_accumulate): what train/train_val.prototxt:1-62 has two LMDB Data layers for.  The bodies are
// csrc/trainset_device.hpp's, which tests/hostsim/sim_trainset.cpp builds for the host unmodified.  Compiled with
// -ffp-contract=off: the transforms round like NumPy's separate ufunc calls.
//   trainset_lines  one thread per output line: its batch slot by bisection of the output offsets, the stored line, the
//                   slot's transform (or a plain copy), three stores
//   trainset_vps    one thread per output VP: likewise, then the label cell and a plain 1.0f store into the slot's map
//   trainset_sum    one thread per pixel: adds the B rasters in index order into the uint32 sum
// All three move a few bytes per thread once: no speed claim is made for them.
#include <string.h>

#include "vpk_internal.hpp"
#include "trainset_device.hpp"

using namespace vpk_trainset;

namespace {

constexpr int THREADS = 256;

// the header of one call, in 8-byte words: [out line offsets B+1 | out VP offsets B+1 | stored first line B | stored first
// VP B | transforms 6 B (only when the call has them)]
struct Header {
    const long long* line_off;
    const long long* vp_off;
    const long long* src_line;
    const long long* src_vp;
    const double* xf;            // NULL: the identity
};

__global__ void __launch_bounds__(THREADS) trainset_lines(Header hd, int B, long long total, const double* __restrict__ l,
                                                          double* __restrict__ l_out) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= total) return;
    const int b = slot_of(hd.line_off, B, t);
    const long long src = hd.src_line[b] + (t - hd.line_off[b]);
    const double in[3] = {l[3 * src], l[3 * src + 1], l[3 * src + 2]};
    double m[3] = {in[0], in[1], in[2]};
    if (hd.xf) transform_line(hd.xf + 6 * b, in, m);
    l_out[3 * t] = m[0];
    l_out[3 * t + 1] = m[1];
    l_out[3 * t + 2] = m[2];
}

__global__ void __launch_bounds__(THREADS) trainset_vps(Header hd, int B, long long total, const double* __restrict__ vps,
                                                        int gh, int gw, double* __restrict__ vp_out,
                                                        int* __restrict__ cell_out, float* __restrict__ labels_out) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= total) return;
    const int b = slot_of(hd.vp_off, B, t);
    const long long src = hd.src_vp[b] + (t - hd.vp_off[b]);
    const double in[3] = {vps[3 * src], vps[3 * src + 1], vps[3 * src + 2]};
    double w[3] = {in[0], in[1], in[2]};
    if (hd.xf) transform_vp(hd.xf + 6 * b, in, w);
    if (vp_out) {
        vp_out[3 * t] = w[0];
        vp_out[3 * t + 1] = w[1];
        vp_out[3 * t + 2] = w[2];
    }
    if (!cell_out && !labels_out) return;
    const int cell = label_cell(w, gh, gw);
    if (cell_out) cell_out[t] = cell;
    if (labels_out && cell >= 0) labels_out[(long long)b * (gh * gw) + cell] = 1.0f;   // two VPs of a cell store the same value
}

__global__ void __launch_bounds__(THREADS) trainset_sum(const uint8_t* __restrict__ rasters, int B, long long P,
                                                        uint32_t* __restrict__ sum) {
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= P) return;
    uint32_t s = sum[p];
    for (int b = 0; b < B; ++b) s += rasters[(long long)b * P + p];
    sum[p] = s;
}

}  // namespace

extern "C" {

int vpk_trainset_batch(vpk_handle* h, const double* l, const int64_t* line_offsets, const double* vps, const int64_t* vp_offsets,
                       int n, const int32_t* index, const double* transforms, int B, const int64_t* out_offsets, int gh, int gw,
                       double* l_out, double* vp_out, int32_t* cell_out, float* labels_out) {
    if (!h) return VPK_ERR_ARG;
    if (!line_offsets || !vp_offsets || !index || !out_offsets)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_batch: the offsets, the index or the output offsets are NULL");
    if (n < 1 || B < 1) return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_batch: n < 1 or B < 1");
    if (gh < 1 || gh > MAX_GRID || gw < 1 || gw > MAX_GRID)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_batch: gh and gw must be 1..64");
    if (out_offsets[0] != 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_batch: out_offsets must start at 0");
    long long n_vps = 0;
    for (int b = 0; b < B; ++b) {
        const int i = index[b];
        if (i < 0 || i >= n) return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_batch: an index is outside 0..n-1");
        const long long lines = line_offsets[i + 1] - line_offsets[i], v = vp_offsets[i + 1] - vp_offsets[i];
        if (lines < 0 || v < 0 || line_offsets[i] < 0 || vp_offsets[i] < 0)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_batch: the store's offsets decrease");
        if (out_offsets[b + 1] - out_offsets[b] != lines)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_batch: out_offsets are not the prefix sums of the chosen images' line counts");
        n_vps += v;
        if (transforms && !affine_valid(transforms + 6 * (size_t)b))
            return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_batch: a transform is not finite or has det == 0");
    }
    const long long n_lines = out_offsets[B];
    const bool want_vps = vp_out || cell_out || labels_out;
    if ((l_out && n_lines > 0 && !l) || (want_vps && n_vps > 0 && !vps))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_batch: the store's lines or VPs are NULL although an output reads them");
    if (n_lines > 0x7fffffffll * THREADS || n_vps > 0x7fffffffll * THREADS)
        return vpk_fail(h, VPK_ERR_LIMIT, "vpk_trainset_batch: more lines or VPs than one launch takes");
    VPK_HIP(h, hipSetDevice(h->device));
    const size_t words = 2 * ((size_t)B + 1) + 2 * (size_t)B + (transforms ? 6 * (size_t)B : 0);
    void* host;
    if (int rc = vpk_stage_begin(h, h->trainset_hdr, words * 8, &host)) return rc;
    long long* w_line = (long long*)host;
    long long* w_vp = w_line + B + 1;
    long long* w_sl = w_vp + B + 1;
    long long* w_sv = w_sl + B;
    w_vp[0] = 0;
    for (int b = 0; b < B; ++b) {
        const int i = index[b];
        w_line[b] = out_offsets[b];
        w_vp[b + 1] = w_vp[b] + (vp_offsets[i + 1] - vp_offsets[i]);
        w_sl[b] = line_offsets[i];
        w_sv[b] = vp_offsets[i];
    }
    w_line[B] = out_offsets[B];
    if (transforms) memcpy(w_sv + B, transforms, 6 * (size_t)B * sizeof(double));
    if (int rc = vpk_stage_commit(h, h->trainset_hdr, words * 8, "vpk_trainset_batch: header")) return rc;
    Header hd;
    hd.line_off = (const long long*)h->trainset_hdr.dev;
    hd.vp_off = hd.line_off + B + 1;
    hd.src_line = hd.vp_off + B + 1;
    hd.src_vp = hd.src_line + B;
    hd.xf = transforms ? (const double*)(hd.src_vp + B) : nullptr;
    if (labels_out) VPK_HIP(h, hipMemsetAsync(labels_out, 0, (size_t)B * gh * gw * sizeof(float), h->stream));
    if (l_out && n_lines > 0) {
        hipLaunchKernelGGL(trainset_lines, dim3((unsigned)((n_lines + THREADS - 1) / THREADS)), dim3(THREADS), 0, h->stream, hd, B,
                           n_lines, l, l_out);
        VPK_HIP(h, hipGetLastError());
    }
    if (want_vps && n_vps > 0) {
        hipLaunchKernelGGL(trainset_vps, dim3((unsigned)((n_vps + THREADS - 1) / THREADS)), dim3(THREADS), 0, h->stream, hd, B,
                           n_vps, vps, gh, gw, vp_out, (int*)cell_out, labels_out);
        VPK_HIP(h, hipGetLastError());
    }
    return VPK_OK;
}

int vpk_trainset_accumulate(vpk_handle* h, const uint8_t* rasters, int B, int64_t P, uint32_t* sum, int64_t* count) {
    if (!h) return VPK_ERR_ARG;
    if (!rasters || !sum || !count) return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_accumulate: a buffer is NULL");
    if (B < 1 || P < 1 || *count < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_trainset_accumulate: B < 1, P < 1 or a negative count");
    if (*count > MAX_MEAN_IMAGES - B)
        return vpk_fail(h, VPK_ERR_LIMIT, "vpk_trainset_accumulate: more than 16843009 images would overflow the uint32 sums");
    if (P > 0x7fffffffll * THREADS) return vpk_fail(h, VPK_ERR_LIMIT, "vpk_trainset_accumulate: more pixels than one launch takes");
    VPK_HIP(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(trainset_sum, dim3((unsigned)((P + THREADS - 1) / THREADS)), dim3(THREADS), 0, h->stream, rasters, B,
                       (long long)P, sum);
    VPK_HIP(h, hipGetLastError());
    *count += B;
    return VPK_OK;
}

}  // extern "C"
