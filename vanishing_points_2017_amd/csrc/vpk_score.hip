// vpk_score.hip -- a benchmark run's scoring on the device (vpk_horizon_error_batch, vpk_auc).  The bodies are
// csrc/score_device.hpp's, which tests/hostsim/sim_score.cpp builds for the host unmodified.  Compiled with
// -ffp-contract=off: the arithmetic rounds like NumPy's.
//   score_errors  one thread per image, grid-stride
//   score_rank    one thread per error, RANK_THREADS errors per workgroup: the errors pass through LDS tile by tile and a
//                 thread counts those that precede its own; it stores its error at that rank
//   score_auc     ONE workgroup: the count of errors up to the cutoff and the crossing (integer reductions), then the
//                 trapezoid sum as AUC_THREADS strided partial sums and a fixed tree in LDS -- no floating-point atomics
// All three are launch-sized: no speed claim is made for them.
#include "vpk_internal.hpp"
#include "score_device.hpp"

using namespace vpk_score;

namespace {

constexpr int ERR_THREADS = 256;
constexpr int ERR_MAX_BLOCKS = 1024;
constexpr int RANK_THREADS = 256;

__global__ void __launch_bounds__(ERR_THREADS) score_errors(int batch, const double* __restrict__ horizon,
                                                            const double* __restrict__ true_horizon,
                                                            const int* __restrict__ dims, double* __restrict__ err) {
    for (long long b = (long long)blockIdx.x * ERR_THREADS + threadIdx.x; b < batch; b += (long long)gridDim.x * ERR_THREADS) {
        const double* o = horizon + b * 15;                   // hP1 at 0..2, hP2 at 3..5
        err[b] = horizon_error(o[1], o[4], true_horizon + b * 3, dims[2 * b], dims[2 * b + 1]);
    }
}

__global__ void __launch_bounds__(RANK_THREADS) score_rank(int n, const double* __restrict__ err, double* __restrict__ sorted) {
    __shared__ double s_tile[RANK_THREADS];
    const int tid = (int)threadIdx.x;
    const int i = (int)blockIdx.x * RANK_THREADS + tid;
    const bool live = i < n;
    const double ei = live ? err[i] : 0.0;
    int rank = 0;
    for (int base = 0; base < n; base += RANK_THREADS) {
        const int j = base + tid;
        s_tile[tid] = j < n ? err[j] : 0.0;
        __syncthreads();
        if (live) {
            const int m = n - base < RANK_THREADS ? n - base : RANK_THREADS;
            for (int q = 0; q < m; ++q) rank += err_precedes(s_tile[q], base + q, ei, i) ? 1 : 0;
        }
        __syncthreads();
    }
    if (live) sorted[rank] = ei;                              // the ranks are a permutation of 0..n-1
}

__global__ void __launch_bounds__(AUC_THREADS) score_auc(int n, const double* __restrict__ sorted, double cutoff,
                                                         double* __restrict__ auc_out) {
    __shared__ int s_below[AUC_THREADS], s_cross[AUC_THREADS];
    __shared__ double s_sum[AUC_THREADS];
    const int t = (int)threadIdx.x;
    auc_scan(sorted, n, cutoff, t, AUC_THREADS, &s_below[t], &s_cross[t]);
    __syncthreads();
    for (int half = AUC_THREADS / 2; half > 0; half /= 2) {
        if (t < half) {
            s_below[t] += s_below[t + half];
            s_cross[t] = s_cross[t] > s_cross[t + half] ? s_cross[t] : s_cross[t + half];   // the last crossing wins
        }
        __syncthreads();
    }
    const int k = s_below[0];
    const double tail_y = auc_tail_y(sorted, n, cutoff, s_cross[0]);
    s_sum[t] = auc_partial(sorted, n, k, cutoff, tail_y, t, AUC_THREADS);
    __syncthreads();
    for (int half = AUC_THREADS / 2; half > 0; half /= 2) {   // auc_tree, one addition per thread and level
        if (t < half) s_sum[t] = s_sum[t] + s_sum[t + half];
        __syncthreads();
    }
    if (t == 0) auc_out[0] = s_sum[0] / cutoff;               // auc.py:37
}

}  // namespace

extern "C" {

int vpk_horizon_error_batch(vpk_handle* h, int batch, const double* horizon, const double* true_horizon, const int32_t* dims,
                            double* err_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_horizon_error_batch: batch < 0");
    if (batch == 0) return VPK_OK;
    if (!horizon || !true_horizon || !dims || !err_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_horizon_error_batch: a buffer is NULL");
    for (int b = 0; b < batch; ++b)
        if (dims[2 * b] < 1 || dims[2 * b + 1] < 1)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_horizon_error_batch: width and height must be >= 1");
    VPK_HIP(h, hipSetDevice(h->device));
    const int rc = vpk_stage_upload(h, h->score_hdr, dims, (size_t)batch * 2 * sizeof(int32_t), "vpk_horizon_error_batch: sizes");
    if (rc) return rc;
    const int want = (batch + ERR_THREADS - 1) / ERR_THREADS;
    const int blocks = want < ERR_MAX_BLOCKS ? want : ERR_MAX_BLOCKS;
    hipLaunchKernelGGL(score_errors, dim3(blocks), dim3(ERR_THREADS), 0, h->stream, batch, horizon, true_horizon,
                       (const int*)h->score_hdr.dev, err_out);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

int vpk_auc(vpk_handle* h, int n, const double* err, double cutoff, double* sorted_out, double* auc_out) {
    if (!h) return VPK_ERR_ARG;
    if (n < 1) return vpk_fail(h, VPK_ERR_ARG, "vpk_auc: n < 1 (the curve needs a last point, auc.py:30)");
    if (n > AUC_MAX_N) return vpk_fail(h, VPK_ERR_LIMIT, "vpk_auc: more than 65536 errors");
    if (!err || !sorted_out || !auc_out || err == sorted_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_auc: a buffer is NULL, or err and sorted_out are the same buffer");
    VPK_HIP(h, hipSetDevice(h->device));
    const int blocks = (n + RANK_THREADS - 1) / RANK_THREADS;
    hipLaunchKernelGGL(score_rank, dim3(blocks), dim3(RANK_THREADS), 0, h->stream, n, err, sorted_out);
    VPK_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(score_auc, dim3(1), dim3(AUC_THREADS), 0, h->stream, n, (const double*)sorted_out, cutoff, auc_out);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // extern "C"
