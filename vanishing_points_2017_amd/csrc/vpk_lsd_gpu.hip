// vpk_lsd_gpu.hip -- batched line segment detection on the GPU (C-ABI entry vpk_lsd_detect_batch).
//
// Per image the same detector as vpk_lsd_detect (csrc/vpk_lsd.cpp), in the same order; the arithmetic is in
// lsd_device.hpp.  Five launches per chunk of images, every image-sized pass grid-wide over the chunk:
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

using namespace vpk_lsd;

namespace {

constexpr int PASS_THREADS = 256;
constexpr int ORDER_THREADS = 1024;
constexpr int ORDER_WAVES = ORDER_THREADS / 64;
constexpr int MAX_CHUNK_IMAGES = 4096;
constexpr size_t DEFAULT_WS_LIMIT = (size_t)4 << 30;
constexpr long long MAX_DIM = 1 << 20;          // input or scaled side
constexpr long long MAX_SCALED_PIXELS = 1 << 30; // seeds are packed as y * xs + x into an int

struct ImgDesc {
    long long in_off;                             // first pixel in `images`
    long long aux, scaled, ang, grad, order, reg, used;   // byte offsets into the chunk's workspace
    int w, h, xs, ys;
    int b;                                        // index in the batch
    int min_reg;
    double logNT;
};

struct Meta {                                     // per image of a chunk, zeroed before it
    unsigned long long max_grad;                  // bits of a non-negative double: integer max = double max
    int n_seeds;
    int pad;
};

inline long long align256(long long v) { return (v + 255) & ~255LL; }

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

// seeds: pixels x < xs - 1, y < ys - 1 whose angle is defined (the host also pushes the others; its seed loop skips them),
// walked in the host's push order c = x * (ys - 1) + y.  Wave w owns a contiguous range of c, so a bin's seeds of wave w
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
    std::vector<ImgDesc> desc((size_t)batch);
    std::vector<long long> bytes((size_t)batch);
    int max_c = 0;
    for (int b = 0; b < batch; ++b) {
        const int w = dims[2 * b], ht = dims[2 * b + 1];
        if (w < 8 || ht < 8) return vpk_fail(h, VPK_ERR_ARG, "vpk_lsd_detect_batch: width and height must be >= 8");
        if (pix_offsets[b + 1] - pix_offsets[b] != (int64_t)w * ht || pix_offsets[b] < 0)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_lsd_detect_batch: pix_offsets do not match width * height");
        if (w > MAX_DIM || ht > MAX_DIM || !((double)w * scale <= (double)MAX_DIM) || !((double)ht * scale <= (double)MAX_DIM))
            return vpk_fail(h, VPK_ERR_LIMIT, "vpk_lsd_detect_batch: image side beyond 2^20 pixels");
        int xs, ys;
        scaled_size(w, ht, scale, xs, ys);
        const long long P = (long long)xs * ys;
        if (P > MAX_SCALED_PIXELS || xs < 1 || ys < 1)
            return vpk_fail(h, VPK_ERR_LIMIT, "vpk_lsd_detect_batch: sub-sampled image beyond 2^30 pixels");
        ImgDesc& d = desc[(size_t)b];
        memset(&d, 0, sizeof(d));
        d.in_off = pix_offsets[b];
        d.w = w; d.h = ht; d.xs = xs; d.ys = ys; d.b = b;
        d.logNT = log_nt(xs, ys);
        d.min_reg = min_reg_size(d.logNT, q.p);
        long long o = 0;
        if (scale != 1.0) {
            d.aux = o; o += align256((long long)xs * ht * 8);
            d.scaled = o; o += align256(P * 8);
            max_c = xs > max_c ? xs : max_c;
            max_c = ys > max_c ? ys : max_c;
        }
        d.ang = o; o += align256(P * 8);
        d.grad = o; o += align256(P * 8);
        d.order = o; o += align256(P * 4);
        d.reg = o; o += align256(P * 8);
        d.used = o; o += align256(P);
        bytes[(size_t)b] = o;
    }
    // chunks: consecutive images while their workspace stays under the limit (at least one image per chunk)
    const size_t limit = h->lsd_ws_limit ? h->lsd_ws_limit : DEFAULT_WS_LIMIT;
    std::vector<int> starts;
    size_t ws_need = 0;
    {
        int b = 0;
        while (b < batch) {
            const int s = b;
            long long used = 0;
            while (b < batch && b - s < MAX_CHUNK_IMAGES) {
                const long long meta = align256((long long)(b - s + 1) * sizeof(Meta));
                if (b > s && meta + used + bytes[(size_t)b] > (long long)limit) break;
                used += bytes[(size_t)b];
                ++b;
            }
            starts.push_back(s);
            // offsets inside the chunk: the Meta array first, then the images one after the other
            const long long meta = align256((long long)(b - s) * sizeof(Meta));
            long long base = meta;
            for (int k = s; k < b; ++k) {
                ImgDesc& d = desc[(size_t)k];
                if (scale != 1.0) { d.aux += base; d.scaled += base; }
                d.ang += base; d.grad += base; d.order += base; d.reg += base; d.used += base;
                base += bytes[(size_t)k];
            }
            if ((size_t)base > ws_need) ws_need = (size_t)base;
        }
        starts.push_back(batch);
    }
    VPK_HIP(h, hipSetDevice(h->device));
    // header: descriptors, then the Gaussian weights of every output coordinate 0..max_c-1
    const size_t desc_bytes = (size_t)align256((long long)batch * sizeof(ImgDesc));
    const size_t hdr_bytes = desc_bytes + (size_t)max_c * q.taps * sizeof(double);
    if (h->lsd_ev_valid) VPK_HIP(h, hipEventSynchronize(h->lsd_ev));  // the previous call's upload has left the staging
    if (h->lsd_host_bytes < hdr_bytes) {
        if (h->lsd_host) VPK_HIP(h, hipHostFree(h->lsd_host));
        h->lsd_host = nullptr;
        h->lsd_host_bytes = 0;
        VPK_HIP(h, hipHostMalloc(&h->lsd_host, hdr_bytes, hipHostMallocDefault));
        h->lsd_host_bytes = hdr_bytes;
    }
    if (!h->lsd_ev) VPK_HIP(h, hipEventCreateWithFlags(&h->lsd_ev, hipEventDisableTiming));
    unsigned char* stage = (unsigned char*)h->lsd_host;
    memcpy(stage, desc.data(), (size_t)batch * sizeof(ImgDesc));
    if (max_c) gaussian_weights((double*)(stage + desc_bytes), max_c, q);
    int rc = vpk_reserve(h, &h->lsd_hdr, &h->lsd_hdr_bytes, hdr_bytes, "vpk_lsd_detect_batch: header");
    if (rc) return rc;
    rc = vpk_reserve(h, &h->lsd_ws, &h->lsd_ws_bytes, ws_need, "vpk_lsd_detect_batch: workspace");
    if (rc) return rc;
    VPK_HIP(h, hipMemcpyAsync(h->lsd_hdr, stage, hdr_bytes, hipMemcpyHostToDevice, h->stream));
    VPK_HIP(h, hipEventRecord(h->lsd_ev, h->stream));
    h->lsd_ev_valid = true;
    const ImgDesc* ddesc = (const ImgDesc*)h->lsd_hdr;
    const double* wts = (const double*)((unsigned char*)h->lsd_hdr + desc_bytes);
    unsigned char* ws = (unsigned char*)h->lsd_ws;
    Meta* meta = (Meta*)ws;
    for (size_t c = 0; c + 1 < starts.size(); ++c) {
        const int s = starts[c], n = starts[c + 1] - s;
        long long max_aux = 0, max_px = 0;
        for (int k = s; k < starts[c + 1]; ++k) {
            const ImgDesc& d = desc[(size_t)k];
            max_aux = (long long)d.xs * d.h > max_aux ? (long long)d.xs * d.h : max_aux;
            max_px = (long long)d.xs * d.ys > max_px ? (long long)d.xs * d.ys : max_px;
        }
        auto blocks = [](long long total) {
            const long long g = (total + PASS_THREADS - 1) / PASS_THREADS;
            return (unsigned)(g < 1024 ? g : 1024);
        };
        VPK_HIP(h, hipMemsetAsync(meta, 0, (size_t)n * sizeof(Meta), h->stream));
        if (scale != 1.0) {
            hipLaunchKernelGGL(lsd_sample_x, dim3(blocks(max_aux), n), dim3(PASS_THREADS), 0, h->stream, ddesc + s, images, wts,
                               q, ws);
            hipLaunchKernelGGL(lsd_sample_y, dim3(blocks(max_px), n), dim3(PASS_THREADS), 0, h->stream, ddesc + s, wts, q, ws);
        }
        if (h->lsd_math == 1)
            hipLaunchKernelGGL(lsd_gradient<Portable>, dim3(blocks(max_px), n), dim3(PASS_THREADS), 0, h->stream, ddesc + s,
                               images, q, ws, meta);
        else
            hipLaunchKernelGGL(lsd_gradient<Libm>, dim3(blocks(max_px), n), dim3(PASS_THREADS), 0, h->stream, ddesc + s,
                               images, q, ws, meta);
        hipLaunchKernelGGL(lsd_order, dim3(n), dim3(ORDER_THREADS), 0, h->stream, ddesc + s, ws, meta);
        if (h->lsd_math == 1)
            hipLaunchKernelGGL(lsd_region<Portable>, dim3(n), dim3(64), 0, h->stream, ddesc + s, q, ws, (const Meta*)meta, out,
                               max_segments, (int*)n_out);
        else
            hipLaunchKernelGGL(lsd_region<Libm>, dim3(n), dim3(64), 0, h->stream, ddesc + s, q, ws, (const Meta*)meta, out,
                               max_segments, (int*)n_out);
        VPK_HIP(h, hipGetLastError());
    }
    return VPK_OK;
}

}  // extern "C"
