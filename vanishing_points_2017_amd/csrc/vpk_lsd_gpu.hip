// vpk_lsd_gpu.hip -- batched line segment detection on the GPU (C-ABI entry vpk_lsd_detect_batch).
//
// Per image the same detector as vpk_lsd_detect, from the same source and in the same order: the arithmetic is in
// lsd_device.hpp (lsd_host.hpp is its serial loop on the host); what is decided on the host before a launch -- the rules,
// the workspace layout, the chunks -- is in lsd_plan.hpp.  Five launches per chunk of images, every image-sized pass
// grid-wide over the chunk:
//   lsd_sample_x    Gaussian sub-sampling along x (input -> aux), weights made on the host by the host's formula
//   lsd_sample_y    ... along y (aux -> scaled)
//   lsd_gradient    gradient, level-line angle, magnitude, per-image max of the magnitudes (exact: a max), `used` cleared
//   lsd_order       per-image stable counting sort of the seeds into 1024 bins, high to low, the host's column-major push
//                   order within a bin (one 1024-thread workgroup per image, one LDS histogram per wave)
//   lsd_region      the seed loop -- region growing, rectangle, refinement, NFA -- one wave per image (lsd_device.hpp)
// The workspace lives on the handle and grows on demand; images are grouped into chunks whose workspace stays under the
// handle's limit (vpk_lsd_set_workspace_limit).  Each image reads and writes only its own slice, so its rows do not depend
// on what else is in the batch or on how the batch was chunked.
// lsd_gradient and lsd_region exist for both math policies of lsd_device.hpp: Libm (the product) and Portable (test-only,
// vpk_lsd_set_math), under which the rows equal the host build's bit for bit.
#include "vpk_internal.hpp"

#include <string.h>

#include "lsd_device.hpp"
#include "lsd_plan.hpp"

using namespace vpk_lsd;

namespace {

constexpr int PASS_THREADS = 256;
constexpr int ORDER_THREADS = 1024;
constexpr int ORDER_WAVES = ORDER_THREADS / 64;

template <class T> __device__ __forceinline__ T* at(unsigned char* ws, long long off) { return (T*)(ws + off); }

__global__ void __launch_bounds__(PASS_THREADS) lsd_sample_x(const ImgDesc* __restrict__ desc, const double* __restrict__ images,
                                                             const double* __restrict__ weights, Params q, unsigned char* ws) {
    const ImgDesc d = desc[blockIdx.y];
    const long long total = (long long)d.xs * d.h;
    double* aux = at<double>(ws, d.aux);
    const double* in = images + d.in_off;
    for (long long i = (long long)blockIdx.x * PASS_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * PASS_THREADS) {
        const int y = (int)(i / d.xs), x = (int)(i % d.xs);
        aux[i] = sample(in + (long long)y * d.w, d.w, 1, x, weights + (long long)x * q.taps, q);
    }
}

__global__ void __launch_bounds__(PASS_THREADS) lsd_sample_y(const ImgDesc* __restrict__ desc, const double* __restrict__ weights,
                                                             Params q, unsigned char* ws) {
    const ImgDesc d = desc[blockIdx.y];
    const long long total = (long long)d.xs * d.ys;
    const double* aux = at<double>(ws, d.aux);
    double* out = at<double>(ws, d.scaled);
    for (long long i = (long long)blockIdx.x * PASS_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * PASS_THREADS) {
        const int y = (int)(i / d.xs), x = (int)(i % d.xs);
        out[i] = sample(aux + x, d.h, d.xs, y, weights + (long long)y * q.taps, q);
    }
}

template <class M>
__global__ void __launch_bounds__(PASS_THREADS) lsd_gradient(const ImgDesc* __restrict__ desc, const double* __restrict__ images,
                                                             Params q, unsigned char* ws, Meta* meta) {
    const ImgDesc d = desc[blockIdx.y];
    const long long total = (long long)d.xs * d.ys;
    const double* img = q.scale != 1.0 ? at<double>(ws, d.scaled) : images + d.in_off;
    double* ang = at<double>(ws, d.ang);
    double* grad = at<double>(ws, d.grad);
    unsigned char* used = at<unsigned char>(ws, d.used);
    double mx = 0.0;
    for (long long i = (long long)blockIdx.x * PASS_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * PASS_THREADS) {
        const int y = (int)(i / d.xs), x = (int)(i % d.xs);
        double a;
        const double g = gradient<M>(img, d.xs, d.ys, x, y, q.rho, &a);
        ang[i] = a;
        grad[i] = g;
        used[i] = 0;
        if (a != NOTDEF && g > mx) mx = g;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_xor(mx, o);
        if (v > mx) mx = v;
    }
    if ((threadIdx.x & 63) == 0 && mx > 0.0)
        atomicMax(&meta[blockIdx.y].max_grad, (unsigned long long)__double_as_longlong(mx));
}

// seeds: pixels x < xs - 1, y < ys - 1 whose angle is defined, walked in the host's push order c = x * (ys - 1) + y
// (lsd_host.hpp).  Wave w owns a contiguous range of c, so a bin's seeds of wave w
// come after those of the waves before it: cursor[w][bin] starts at the bin's start plus their counts.
__global__ void __launch_bounds__(ORDER_THREADS) lsd_order(const ImgDesc* __restrict__ desc, unsigned char* ws, Meta* meta) {
    __shared__ int hist[ORDER_WAVES][N_BINS];
    __shared__ int scan[N_BINS];
    const ImgDesc d = desc[blockIdx.x];
    const double* ang = at<double>(ws, d.ang);
    const double* grad = at<double>(ws, d.grad);
    int* order = at<int>(ws, d.order);
    const double mg = __longlong_as_double((long long)meta[blockIdx.x].max_grad);
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int ny = d.ys - 1;
    const long long C = (long long)(d.xs - 1) * ny;
    const long long seg = ((C + ORDER_WAVES - 1) / ORDER_WAVES + 63) & ~63LL;
    const long long c0 = seg * wv, c1 = c0 + seg < C ? c0 + seg : C;
    for (int k = tid; k < ORDER_WAVES * N_BINS; k += ORDER_THREADS) (&hist[0][0])[k] = 0;
    __syncthreads();
    if (!(mg > 0.0)) {                            // no pixel above the threshold: no seed
        if (tid == 0) meta[blockIdx.x].n_seeds = 0;
        return;
    }
    for (long long c = c0 + lane; c < c1; c += 64) {
        const int x = (int)(c / ny), y = (int)(c % ny);
        const long long adr = (long long)y * d.xs + x;
        if (ang[adr] != NOTDEF) atomicAdd(&hist[wv][grad_bin(grad[adr], mg)], 1);
    }
    __syncthreads();
    // bins from high to low: rank r = N_BINS - 1 - bin; exclusive prefix over r of the bin totals
    const int bin = N_BINS - 1 - tid;
    int tot = 0;
    for (int w = 0; w < ORDER_WAVES; ++w) tot += hist[w][bin];
    scan[tid] = tot;
    __syncthreads();
    for (int o = 1; o < N_BINS; o <<= 1) {
        const int v = tid >= o ? scan[tid - o] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    int run = scan[tid] - tot;
    if (tid == N_BINS - 1) meta[blockIdx.x].n_seeds = scan[tid];
    for (int w = 0; w < ORDER_WAVES; ++w) {
        const int cnt = hist[w][bin];
        hist[w][bin] = run;
        run += cnt;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long long cb = c0; cb < c1; cb += 64) {
        const long long c = cb + lane;
        int b = -1, pix = 0;
        if (c < c1) {
            const int x = (int)(c / ny), y = (int)(c % ny);
            const long long adr = (long long)y * d.xs + x;
            if (ang[adr] != NOTDEF) {
                b = grad_bin(grad[adr], mg);
                pix = (int)adr;
            }
        }
        const bool valid = b >= 0;
        unsigned long long same = __ballot(valid);
        for (int k = 0; k < 10; ++k) {            // lanes with the same bin
            const bool bit = valid && ((b >> k) & 1);
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        if (valid) {
            const int rank = __popcll(same & below), cnt = __popcll(same);
            const int pos = hist[wv][b] + rank;
            order[pos] = pix;
            if (rank == cnt - 1) hist[wv][b] = pos + 1;
        }
    }
}

struct DevWave {
    __device__ int lane() const { return (int)(threadIdx.x & 63); }
    __device__ int size() const { return 64; }
    __device__ int sum_int(int v) const {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        return v;
    }
    __device__ double max_d(double v) const {
        for (int o = 32; o > 0; o >>= 1) {
            const double u = __shfl_xor(v, o);
            if (u > v) v = u;
        }
        return v;
    }
    __device__ double min_d(double v) const {
        for (int o = 32; o > 0; o >>= 1) {
            const double u = __shfl_xor(v, o);
            if (u < v) v = u;
        }
        return v;
    }
};

template <class M>
__global__ void __launch_bounds__(64) lsd_region(const ImgDesc* __restrict__ desc, Params q, unsigned char* ws, const Meta* meta,
                                                 double* out, int max_segments, int* n_out) {
    const ImgDesc d = desc[blockIdx.x];
    DevWave w;
    Region<DevWave, M> r{w, at<double>(ws, d.ang), at<double>(ws, d.grad), at<unsigned char>(ws, d.used), at<Pt>(ws, d.reg),
                      d.xs, d.ys, d.logNT};
    const int n = r.detect(at<int>(ws, d.order), meta[blockIdx.x].n_seeds, q, d.min_reg,
                           out + (long long)d.b * max_segments * 7, max_segments);
    if (threadIdx.x == 0) n_out[d.b] = n;
}

// the launches of one chunk of n images (desc: its descriptors on the device); max_aux, max_px: its largest xs * h, xs * ys
template <class M>
void launch_chunk(hipStream_t stream, const ImgDesc* desc, int n, long long max_aux, long long max_px, const double* images,
                  const double* wts, const Params& q, unsigned char* ws, Meta* meta, double* out, int max_segments, int* n_out) {
    auto blocks = [](long long total) {
        const long long g = (total + PASS_THREADS - 1) / PASS_THREADS;
        return (unsigned)(g < 1024 ? g : 1024);
    };
    if (q.scale != 1.0) {
        hipLaunchKernelGGL(lsd_sample_x, dim3(blocks(max_aux), n), dim3(PASS_THREADS), 0, stream, desc, images, wts, q, ws);
        hipLaunchKernelGGL(lsd_sample_y, dim3(blocks(max_px), n), dim3(PASS_THREADS), 0, stream, desc, wts, q, ws);
    }
    hipLaunchKernelGGL(lsd_gradient<M>, dim3(blocks(max_px), n), dim3(PASS_THREADS), 0, stream, desc, images, q, ws, meta);
    hipLaunchKernelGGL(lsd_order, dim3(n), dim3(ORDER_THREADS), 0, stream, desc, ws, meta);
    hipLaunchKernelGGL(lsd_region<M>, dim3(n), dim3(64), 0, stream, desc, q, ws, (const Meta*)meta, out, max_segments, n_out);
}

}  // namespace

extern "C" {

int vpk_lsd_set_workspace_limit(vpk_handle* h, size_t bytes) {
    if (!h) return VPK_ERR_ARG;
    h->lsd_ws_limit = bytes;
    return VPK_OK;
}

int vpk_lsd_set_math(vpk_handle* h, int mode) {
    if (!h) return VPK_ERR_ARG;
    if (mode != 0 && mode != 1) return vpk_fail(h, VPK_ERR_ARG, "vpk_lsd_set_math: mode must be 0 or 1");
    h->lsd_math = mode;
    return VPK_OK;
}

int vpk_lsd_detect_batch(vpk_handle* h, int batch, const int32_t* dims, const int64_t* pix_offsets, const double* images,
                         double scale, double* out, int max_segments, int32_t* n_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0 || (batch > 0 && (!dims || !pix_offsets || !images || !n_out)) || max_segments < 0 ||
        (max_segments > 0 && !out) || !(scale > 0.0))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_lsd_detect_batch: bad argument");
    if (batch == 0) return VPK_OK;
    const Params q = make_params(scale);
    const Plan plan = plan_batch(batch, dims, pix_offsets, scale, h->lsd_ws_limit);
    if (plan.rule) {
        static const char* const what[] = {nullptr,
                                           "vpk_lsd_detect_batch: width and height must be >= 8",            // PLAN_SIDE
                                           "vpk_lsd_detect_batch: pix_offsets do not match width * height",  // PLAN_OFFSETS
                                           "vpk_lsd_detect_batch: image side beyond 2^20 pixels",            // PLAN_DIM
                                           "vpk_lsd_detect_batch: sub-sampled image beyond 2^30 pixels"};    // PLAN_PIXELS
        return vpk_fail(h, plan_code(plan.rule), what[plan.rule]);
    }
    VPK_HIP(h, hipSetDevice(h->device));
    // header: descriptors, then the Gaussian weights of every output coordinate 0..max_c-1
    const size_t desc_bytes = (size_t)align256((long long)batch * sizeof(ImgDesc));
    const size_t hdr_bytes = desc_bytes + (size_t)plan.max_c * q.taps * sizeof(double);
    void* host;
    if (int rc = vpk_stage_begin(h, h->lsd_hdr, hdr_bytes, &host)) return rc;
    unsigned char* stage = (unsigned char*)host;
    memcpy(stage, plan.desc.data(), (size_t)batch * sizeof(ImgDesc));
    if (plan.max_c) gaussian_weights((double*)(stage + desc_bytes), plan.max_c, q);
    if (int rc = vpk_stage_commit(h, h->lsd_hdr, hdr_bytes, "vpk_lsd_detect_batch: header")) return rc;
    if (int rc = vpk_reserve(h, &h->lsd_ws, &h->lsd_ws_bytes, plan.ws_bytes, "vpk_lsd_detect_batch: workspace")) return rc;
    const ImgDesc* ddesc = (const ImgDesc*)h->lsd_hdr.dev;
    const double* wts = (const double*)((unsigned char*)h->lsd_hdr.dev + desc_bytes);
    unsigned char* ws = (unsigned char*)h->lsd_ws;
    Meta* meta = (Meta*)ws;
    for (size_t c = 0; c + 1 < plan.starts.size(); ++c) {
        const int s = plan.starts[c], n = plan.starts[c + 1] - s;
        long long max_aux = 0, max_px = 0;
        for (int k = s; k < s + n; ++k) {
            const ImgDesc& d = plan.desc[(size_t)k];
            max_aux = (long long)d.xs * d.h > max_aux ? (long long)d.xs * d.h : max_aux;
            max_px = (long long)d.xs * d.ys > max_px ? (long long)d.xs * d.ys : max_px;
        }
        VPK_HIP(h, hipMemsetAsync(meta, 0, (size_t)n * sizeof(Meta), h->stream));
        switch (h->lsd_math) {
            case 1:
                launch_chunk<Portable>(h->stream, ddesc + s, n, max_aux, max_px, images, wts, q, ws, meta, out, max_segments,
                                       (int*)n_out);
                break;
            default:
                launch_chunk<Libm>(h->stream, ddesc + s, n, max_aux, max_px, images, wts, q, ws, meta, out, max_segments,
                                   (int*)n_out);
        }
        VPK_HIP(h, hipGetLastError());
    }
    return VPK_OK;
}

}  // extern "C"
