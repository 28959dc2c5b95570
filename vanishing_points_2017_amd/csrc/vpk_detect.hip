// vpk_detect.hip -- the two steps that kept a detector's flow on the host between the EM and its results
// (vpk_vp_order_batch, vpk_to_pixels_batch).  The bodies are csrc/detect_device.hpp's, which tests/hostsim/sim_detect.cpp
// builds for the host unmodified.  Compiled with -ffp-contract=off: the pixel arithmetic rounds like NumPy's.
//   det_order      one wave per image, one lane per VP, ORDER_WAVES images per workgroup: a lane's rank is the number of
//                  VPs that precede it (counts read from LDS), lanes with rank < maxbest store their index
//   det_to_pixels  one thread per output row (segments, then VPs, then horizon end points), grid-stride
// Both are launch-sized: no speed claim is made for them.
#include "vpk_internal.hpp"
#include "detect_device.hpp"

#include <string.h>

using namespace vpk_det;

namespace {

constexpr int ORDER_WAVES = 4;
constexpr int ORDER_THREADS = 64 * ORDER_WAVES;
constexpr int PX_THREADS = 256;
constexpr int PX_MAX_BLOCKS = 4096;

__global__ void __launch_bounds__(ORDER_THREADS) det_order(int batch, int max_vp, const double* __restrict__ counts,
                                                           const int* __restrict__ num_vp, int maxbest,
                                                           int* __restrict__ order) {
    __shared__ double s_cnt[ORDER_WAVES][MAX_VP];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const long long b = (long long)blockIdx.x * ORDER_WAVES + wave;
    const bool live = b < batch;
    const int M = live ? clamp_num_vp(num_vp[b], max_vp) : 0;
    if (lane < M) s_cnt[wave][lane] = counts[b * max_vp + lane];
    __syncthreads();
    if (!live) return;
    const int nb = M < maxbest ? M : maxbest;
    int* o = order + b * maxbest;
    if (lane >= nb && lane < maxbest) o[lane] = 0;            // padding: what calculate_horizon_batch uploads
    if (lane < M) {
        const int rank = vp_rank(s_cnt[wave], M, lane);
        if (rank < maxbest) o[rank] = lane;                   // ranks are a permutation of 0..M-1: rank < nb here
    }
}

// header of det_to_pixels: off[0..batch] (int64 line offsets), then dims[2 batch] (int32 w, h)
__global__ void __launch_bounds__(PX_THREADS) det_to_pixels(int batch, const long long* __restrict__ off,
                                                            const int* __restrict__ dims, const double* __restrict__ lp,
                                                            int max_vp, const double* __restrict__ vp,
                                                            const int* __restrict__ num_vp, const double* __restrict__ horizon,
                                                            long long n_lp, long long n_vp, long long n_hz,
                                                            double* __restrict__ lp_px, double* __restrict__ vp_px,
                                                            double* __restrict__ hz_px) {
    const long long total = n_lp + n_vp + n_hz;
    for (long long r = (long long)blockIdx.x * PX_THREADS + threadIdx.x; r < total; r += (long long)gridDim.x * PX_THREADS) {
        if (r < n_lp) {                                       // segment row off[0] + r
            const long long row = off[0] + r;
            int lo = 0, hi = batch;                           // the image b with off[b] <= row < off[b + 1]
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if (off[mid] <= row) lo = mid; else hi = mid;
            }
            segment_to_px(lp + row * 4, dims[2 * lo], dims[2 * lo + 1], lp_px + row * 4);
        } else if (r < n_lp + n_vp) {                         // VP k of image b
            const long long q = r - n_lp;
            const int b = (int)(q / max_vp), k = (int)(q % max_vp);
            double* o = vp_px + q * 2;
            if (k < clamp_num_vp(num_vp[b], max_vp)) vp_to_px(vp + q * 3, dims[2 * b], dims[2 * b + 1], o);
            else o[0] = o[1] = quiet_nan();
        } else {                                              // end point e (hP1, hP2) of image b
            const long long q = r - n_lp - n_vp;
            const int b = (int)(q / 2), e = (int)(q % 2);
            const double* p = horizon + (long long)b * 15 + 3 * e;
            point_to_px(p[0], p[1], dims[2 * b], dims[2 * b + 1], hz_px + q * 2);
        }
    }
}

}  // namespace

extern "C" {

int vpk_vp_order_batch(vpk_handle* h, int batch, int max_vp, const double* counts, const int32_t* num_vp, int maxbest,
                       int32_t* order_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0 || max_vp < 1 || max_vp > MAX_VP || maxbest < 1 || maxbest > MAX_VP)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_vp_order_batch: bad argument (batch >= 0, max_vp and maxbest in 1..64)");
    if (batch == 0) return VPK_OK;
    if (!counts || !num_vp || !order_out) return vpk_fail(h, VPK_ERR_ARG, "vpk_vp_order_batch: a buffer is NULL");
    VPK_HIP(h, hipSetDevice(h->device));
    const int blocks = (batch + ORDER_WAVES - 1) / ORDER_WAVES;
    hipLaunchKernelGGL(det_order, dim3(blocks), dim3(ORDER_THREADS), 0, h->stream, batch, max_vp, counts, (const int*)num_vp,
                       maxbest, (int*)order_out);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

int vpk_to_pixels_batch(vpk_handle* h, int batch, const int32_t* dims, const int64_t* line_offsets, const double* lp,
                        int max_vp, const double* vp, const int32_t* num_vp, const double* horizon, double* lp_px_out,
                        double* vp_px_out, double* horizon_px_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_to_pixels_batch: batch < 0");
    if (batch == 0 || (!lp_px_out && !vp_px_out && !horizon_px_out)) return VPK_OK;
    if (!dims) return vpk_fail(h, VPK_ERR_ARG, "vpk_to_pixels_batch: dims is NULL");
    for (int b = 0; b < batch; ++b)
        if (dims[2 * b] < 1 || dims[2 * b + 1] < 1)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_to_pixels_batch: width and height must be >= 1");
    long long n_lp = 0, n_vp = 0, n_hz = 0;
    if (lp_px_out) {
        if (!line_offsets) return vpk_fail(h, VPK_ERR_ARG, "vpk_to_pixels_batch: lp_px_out without line_offsets");
        if (line_offsets[0] < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_to_pixels_batch: line_offsets[0] < 0");
        for (int b = 0; b < batch; ++b)
            if (line_offsets[b + 1] < line_offsets[b])
                return vpk_fail(h, VPK_ERR_ARG, "vpk_to_pixels_batch: line_offsets decrease");
        n_lp = (long long)(line_offsets[batch] - line_offsets[0]);
        if (n_lp > 0 && !lp) return vpk_fail(h, VPK_ERR_ARG, "vpk_to_pixels_batch: lp_px_out without lp");
    }
    if (vp_px_out) {
        if (max_vp < 1 || max_vp > MAX_VP || !vp || !num_vp)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_to_pixels_batch: vp_px_out needs vp, num_vp and max_vp in 1..64");
        n_vp = (long long)batch * max_vp;
    }
    if (horizon_px_out) {
        if (!horizon) return vpk_fail(h, VPK_ERR_ARG, "vpk_to_pixels_batch: horizon_px_out without horizon");
        n_hz = 2LL * batch;
    }
    const long long total = n_lp + n_vp + n_hz;
    if (total == 0) return VPK_OK;
    // header: line offsets (zeros when no segment is converted), then the sizes
    const size_t off_bytes = ((size_t)batch + 1) * sizeof(int64_t);
    std::vector<unsigned char> hdr(off_bytes + (size_t)batch * 2 * sizeof(int32_t), 0);
    if (lp_px_out) memcpy(hdr.data(), line_offsets, off_bytes);
    memcpy(hdr.data() + off_bytes, dims, (size_t)batch * 2 * sizeof(int32_t));
    VPK_HIP(h, hipSetDevice(h->device));
    const int rc = vpk_stage_upload(h, h->detect_hdr, hdr.data(), hdr.size(), "vpk_to_pixels_batch: header");
    if (rc) return rc;
    const long long* doff = (const long long*)h->detect_hdr.dev;
    const int* ddims = (const int*)((const unsigned char*)h->detect_hdr.dev + off_bytes);
    const long long want = (total + PX_THREADS - 1) / PX_THREADS;
    const int blocks = (int)(want < PX_MAX_BLOCKS ? want : PX_MAX_BLOCKS);
    hipLaunchKernelGGL(det_to_pixels, dim3(blocks), dim3(PX_THREADS), 0, h->stream, batch, doff, ddims, lp, max_vp, vp,
                       (const int*)num_vp, horizon, n_lp, n_vp, n_hz, lp_px_out, vp_px_out, horizon_px_out);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // extern "C"
