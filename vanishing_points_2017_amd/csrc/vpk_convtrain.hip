// vpk_convtrain.hip -- SGD fine-tuning of the conv stack (conv1-5, LRN, the pools) on float32 master weights.
//
// One step (train/train_val.prototxt:66-288 under train/solver.prototxt), around the head's vpk_train_step_dx:
//   forward    per layer one launch: convolution as a gathered product on the f32 matrix cores (ct_gemm<GEMM_FWD>), LRN with
//              the channel column of 32 pixels in LDS (ct_lrn_fwd), MAX pooling with its argmax (ct_pool_fwd)
//   backward   pools by a gather over the windows that contain an element (ct_pool_bwd), LRN (ct_lrn_bwd), convolutions:
//              dX from the old weights (ct_gemm<GEMM_DGRAD>), then dW and db in slabs of the reduction over (b, y, x)
//              (ct_gemm<GEMM_WGRAD>: db is one more column of the same product), then the slabs' sums in slab order
//              inside Caffe's update of W, b and their momentum (ct_update)
// No dW buffer beyond the slabs' partials and no float atomic: two runs from the same state give the same bits.
// Arithmetic: f32 operands, f32 accumulation (v_mfma_f32_32x32x2_f32 is an exact fmaf chain).  The index maps and the
// per-element rules are convtrain_device.hpp's; the update is train_device.hpp's.
// What the host decides lives elsewhere: the tile constants, the shapes and limits of a chain, the grids, the slab split and
// buffer sizes, the kept blobs' life cycle, the solver's rates and the set_params rule in train_plan.hpp (host-tested); the
// weights, momentum, iteration and their load / store entry points in train_store.hpp, shared with vpk_train.hip.  Here
// are the kernels, the launches and the refusals of forward, backward and read.
#include "vpk_internal.hpp"
#include "convtrain_device.hpp"
#include "train_device.hpp"
#include "train_plan.hpp"
#include "train_store.hpp"

#include <string.h>
#include <vector>

namespace ct = vpk_convtrain;
using namespace vpk_train_plan;

namespace {

typedef float ct_f32x16 __attribute__((ext_vector_type(16)));

// C[m][n] = sum_r A(m, r) B(r, n) of one channel group and one slab of r, gathered through convtrain_device.hpp's maps.
// grid: (tiles of n, tiles of m, groups x slabs).  Per chunk of CT_CHUNK terms the workgroup stages A as As[r][m] and B as
// Bs[r][n] (zeros past the edges), and each wave issues CT_CHUNK / 2 MFMAs on its quadrant: lane l feeds A[m = l & 31]
// [k = l >> 5] and B[k = l >> 5][n = l & 31].  The accumulator's register v of lane l is row (v & 3) + 8 (v >> 2) + 4 (l >> 5),
// column l & 31.
template <int MODE>
__global__ __launch_bounds__(256) void ct_gemm(ct::ConvPtrs p, ct::ConvGeom q, int slabs, int slab_len) {
    __shared__ float As[CT_CHUNK][CT_LDS_ROW];
    __shared__ float Bs[CT_CHUNK][CT_LDS_ROW];
    int M, N, R;
    ct::gemm_dims(MODE, q, M, N, R);
    const int g = blockIdx.z / slabs, slab = blockIdx.z - g * slabs;
    const int n0 = blockIdx.x * CT_TILE, m0 = blockIdx.y * CT_TILE;
    const int r_begin = slab * slab_len, r_end = min(R, r_begin + slab_len);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    ct_f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    for (int r0 = r_begin; r0 < r_end; r0 += CT_CHUNK) {
#pragma unroll
        for (int i = 0; i < CT_TILE * CT_CHUNK / 256; ++i) {
            const int e = tid + 256 * i;
            // A: the weights run along r (FWD) and so does dY (WGRAD); the data gradient's weights run along neither
            const int ar = e % CT_CHUNK, am = e / CT_CHUNK;
            As[ar][am] = (m0 + am < M && r0 + ar < r_end) ? ct::gemm_a(MODE, p, q, g, m0 + am, r0 + ar) : 0.f;
            // B: pixels run along n (FWD, DGRAD) or along r (WGRAD)
            const int br = MODE == ct::GEMM_WGRAD ? e % CT_CHUNK : e / CT_TILE;
            const int bn = MODE == ct::GEMM_WGRAD ? e / CT_CHUNK : e % CT_TILE;
            Bs[br][bn] = (n0 + bn < N && r0 + br < r_end) ? ct::gemm_b(MODE, p, q, g, r0 + br, n0 + bn) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < CT_CHUNK; k2 += 2) {
            const float a = As[k2 + (lane >> 5)][wm + (lane & 31)];
            const float b = Bs[k2 + (lane >> 5)][wn + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int m = m0 + wm + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5), n = n0 + wn + (lane & 31);
        if (m < M && n < N) ct::gemm_store(MODE, p, q, g, slab, m, n, acc[v]);
    }
}

// dW[oc][n] (n < cols - 1) and db[oc] (n = cols - 1) = the slabs' partials added in slab order; then Caffe's update in place
__global__ void ct_update(float* __restrict__ W, float* __restrict__ V, float* __restrict__ bias, float* __restrict__ vb,
                          const float* __restrict__ partial, int slabs, int OC, int cols, float lr_w, float dec_w, float lr_b,
                          float dec_b, float mu) {
    const size_t total = (size_t)OC * cols, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float g = 0.f;
#pragma unroll 4
    for (int t = 0; t < slabs; ++t) g += partial[(size_t)t * total + i];
    const int oc = (int)(i / cols), n = (int)(i - (size_t)oc * cols);
    if (n < cols - 1) {
        const size_t j = (size_t)oc * (cols - 1) + n;
        float w = W[j], v = V[j];
        vpk_train::sgd_update(w, v, g, lr_w, dec_w, mu);
        W[j] = w;
        V[j] = v;
    } else {
        float w = bias[oc], v = vb[oc];
        vpk_train::sgd_update(w, v, g, lr_b, dec_b, mu);
        bias[oc] = w;
        vb[oc] = v;
    }
}

// LRN forward: a workgroup takes CT_LRN_PIX pixels of one image and every channel; col[c][pixel] in LDS.
// grid: (pixel tiles, B).  Thread (pixel = tid & 31, lane = tid >> 5) takes channels lane, lane + 8, ...
__global__ __launch_bounds__(256) void ct_lrn_fwd(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ scale,
                                                  int C, int P, int n, float alpha_over_n, float beta, float k) {
    extern __shared__ float col[];
    const int px = threadIdx.x & (CT_LRN_PIX - 1), cl = threadIdx.x / CT_LRN_PIX;
    const int pix = blockIdx.x * CT_LRN_PIX + px;
    const size_t base = (size_t)blockIdx.y * C * P + pix;
    if (pix < P)
        for (int c = cl; c < C; c += 256 / CT_LRN_PIX) col[c * CT_LRN_PIX + px] = x[base + (size_t)c * P];
    __syncthreads();
    if (pix >= P) return;
    for (int c = cl; c < C; c += 256 / CT_LRN_PIX) {
        const float s = ct::lrn_scale(col + px, CT_LRN_PIX, c, C, n, alpha_over_n, k);
        scale[base + (size_t)c * P] = s;
        y[base + (size_t)c * P] = ct::lrn_forward(col[c * CT_LRN_PIX + px], s, beta);
    }
}

// LRN backward: the column of dy_j y_j / s_j in LDS, then one element per thread and channel step
__global__ __launch_bounds__(256) void ct_lrn_bwd(const float* __restrict__ x, const float* __restrict__ y,
                                                  const float* __restrict__ scale, const float* __restrict__ dy,
                                                  float* __restrict__ dx, int C, int P, int n, float beta, float coef) {
    extern __shared__ float col[];
    const int px = threadIdx.x & (CT_LRN_PIX - 1), cl = threadIdx.x / CT_LRN_PIX;
    const int pix = blockIdx.x * CT_LRN_PIX + px;
    const size_t base = (size_t)blockIdx.y * C * P + pix;
    if (pix < P)
        for (int c = cl; c < C; c += 256 / CT_LRN_PIX) {
            const size_t i = base + (size_t)c * P;
            col[c * CT_LRN_PIX + px] = ct::lrn_ratio(dy[i], y[i], scale[i]);
        }
    __syncthreads();
    if (pix >= P) return;
    for (int c = cl; c < C; c += 256 / CT_LRN_PIX) {
        const size_t i = base + (size_t)c * P;
        dx[i] = ct::lrn_backward(col + px, CT_LRN_PIX, c, C, n, dy[i], x[i], scale[i], beta, coef);
    }
}

// MAX pooling: one output per thread; planes = B x C
__global__ void ct_pool_fwd(const float* __restrict__ x, float* __restrict__ y, int32_t* __restrict__ idx, size_t planes, int H,
                            int W, int OH, int OW, int K, int stride) {
    const size_t total = planes * OH * OW, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t plane = i / ((size_t)OH * OW);
    const int o = (int)(i - plane * OH * OW), oh = o / OW, ow = o - oh * OW;
    int h0, h1, w0, w1;
    ct::pool_window(oh, K, stride, H, h0, h1);
    ct::pool_window(ow, K, stride, W, w0, w1);
    const float* src = x + plane * H * W;
    const int best = ct::pool_argmax(src, W, h0, h1, w0, w1);
    idx[i] = best;
    y[i] = src[best];
}

// its backward: one input element per thread, the windows that contain it in row-major window order
__global__ void ct_pool_bwd(const float* __restrict__ dy, const int32_t* __restrict__ idx, float* __restrict__ dx, size_t planes,
                            int H, int W, int OH, int OW, int K, int stride) {
    const size_t total = planes * H * W, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t plane = i / ((size_t)H * W);
    const int at = (int)(i - plane * H * W), h = at / W, w = at - h * W;
    int oh0, oh1, ow0, ow1;
    ct::pool_windows_of(h, K, stride, OH, oh0, oh1);
    ct::pool_windows_of(w, K, stride, OW, ow0, ow1);
    const size_t ob = plane * OH * OW;
    float s = 0.f;
    for (int oh = oh0; oh <= oh1; ++oh)
        for (int ow = ow0; ow <= ow1; ++ow) {
            const size_t o = ob + (size_t)oh * OW + ow;
            if (idx[o] == at) s += dy[o];
        }
    dx[i] = s;
}

struct ct_layer : LayerShape {
    int blob = -1;                                                      // CONV: its weight in the store, the bias behind it
    float *out = nullptr, *grad = nullptr, *scale = nullptr;            // cap x OC x OH x OW (scale: LRN)
    int32_t* idx = nullptr;                                             // POOL
};

template <int MODE>
void launch_gemm(hipStream_t st, const ct::ConvPtrs& p, const ct::ConvGeom& q, int slabs, int slab_len) {
    const Grid g = gemm_grid(MODE, q, slabs);
    ct_gemm<MODE><<<dim3(g.x, g.y, g.z), 256, 0, st>>>(p, q, slabs, slab_len);
}

}  // namespace

struct vpk_convtrain_state {
    int C = 0, H = 0, W = 0;
    std::vector<ct_layer> L;
    vpk_param_store ps;               // [W, b] of every CONV layer in stack order, and their momentum
    float* xin = nullptr;             // the forward's copy of X: cap x C x H x W
    int cap = 0;                      // images the blobs are allocated for
    KeptBlobs kept;                   // what the blobs hold and who may use it (train_plan.hpp)
    float* partial = nullptr;         // the weight gradient's slabs
    size_t partial_bytes = 0;
    size_t in_size() const { return (size_t)C * H * W; }
};

namespace {

vpk_param_store* store_of(const vpk_handle* h) { return h && h->convtrain ? &h->convtrain->ps : nullptr; }

void free_blobs(vpk_convtrain_state* s) {
    for (ct_layer& L : s->L) {
        for (void* p : {(void*)L.out, (void*)L.grad, (void*)L.scale, (void*)L.idx})
            if (p) (void)hipFree(p);
        L.out = L.grad = L.scale = nullptr;
        L.idx = nullptr;
    }
    if (s->xin) (void)hipFree(s->xin);
    s->xin = nullptr;
    s->cap = 0;
}

int reserve_blobs(vpk_handle* h, vpk_convtrain_state* s, int B) {
    if (B <= s->cap) return VPK_OK;
    VPK_HIP(h, hipStreamSynchronize(h->stream));
    free_blobs(s);
    hipError_t e = hipSuccess;
    auto alloc = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    alloc((void**)&s->xin, (size_t)B * s->in_size() * 4);
    for (ct_layer& L : s->L) {
        alloc((void**)&L.out, blob_bytes(L, B));
        alloc((void**)&L.grad, blob_bytes(L, B));
        if (L.d.kind == VPK_LAYER_LRN) alloc((void**)&L.scale, blob_bytes(L, B));
        if (L.d.kind == VPK_LAYER_POOL) alloc((void**)&L.idx, blob_bytes(L, B));
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        free_blobs(s);
        return vpk_fail_hip(h, e, "vpk_convtrain_forward: hipMalloc of the blobs");
    }
    s->cap = B;
    return VPK_OK;
}

}  // namespace

void vpk_convtrain_free(vpk_handle* h) {
    vpk_convtrain_state* s = h->convtrain;
    if (!s) return;
    (void)hipStreamSynchronize(h->stream);
    free_blobs(s);
    s->ps.free();
    if (s->partial) (void)hipFree(s->partial);
    delete s;
    h->convtrain = nullptr;
}

extern "C" {

int vpk_convtrain_net_layers(vpk_stack_layer* out, int capacity, int32_t in_shape[3]) {
    auto conv = [](int oc, int k, int stride, int pad, int groups) {
        vpk_stack_layer d = {};
        d.kind = VPK_LAYER_CONV;
        d.out_channels = oc; d.kernel = k; d.stride = stride; d.pad = pad; d.groups = groups; d.relu = 1;
        return d;
    };
    auto lrn = []() {
        vpk_stack_layer d = {};
        d.kind = VPK_LAYER_LRN;
        d.local_size = 5; d.alpha = 1e-4f; d.beta = 0.75f; d.k = 1.0f;        // train_val.prototxt:105-107, 161-163; k: Caffe's default
        return d;
    };
    auto pool = []() {
        vpk_stack_layer d = {};
        d.kind = VPK_LAYER_POOL;
        d.kernel = 3; d.stride = 2;                                         // :116-118, 172-174, 284-286
        return d;
    };
    const vpk_stack_layer net[10] = {
        conv(96, 11, 4, 0, 1), lrn(), pool(),        // conv1 :66-92, relu1, norm1, pool1
        conv(256, 5, 1, 2, 2), lrn(), pool(),        // conv2 :121-148, relu2, norm2, pool2
        conv(384, 3, 1, 1, 1),                       // conv3 :177-203, relu3
        conv(384, 3, 1, 1, 2),                       // conv4 :210-237, relu4
        conv(256, 3, 1, 1, 2), pool(),               // conv5 :244-271, relu5, pool5
    };
    if (in_shape) { in_shape[0] = 1; in_shape[1] = 500; in_shape[2] = 500; }
    if (out)
        for (int i = 0; i < 10 && i < capacity; ++i) out[i] = net[i];
    return 10;
}

int vpk_convtrain_create(vpk_handle* h, int C, int H, int W, const vpk_stack_layer* layers, int n_layers) {
    if (!h) return VPK_ERR_ARG;
    if (h->convtrain) return vpk_fail(h, VPK_ERR_STATE, "vpk_convtrain_create: the handle already has a conv trainer");
    std::vector<LayerShape> shapes;
    const StackRule rule = chain(C, H, W, layers, n_layers, shapes);
    if (rule == STACK_NO_CHAIN)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_convtrain_create: the layers do not chain on this input shape");
    if (rule == STACK_LRN_WIDE) return vpk_fail(h, VPK_ERR_LIMIT, "vpk_convtrain_create: an LRN on more than 512 channels");
    VPK_HIP(h, hipSetDevice(h->device));
    vpk_convtrain_state* s = new vpk_convtrain_state();
    h->convtrain = s;
    s->C = C; s->H = H; s->W = W;
    static_assert(2 * CT_MAX_LAYERS <= vpk_param_store::MAX_BLOBS, "a weight and a bias per layer");
    size_t counts[2 * CT_MAX_LAYERS];
    int blobs = 0;
    for (const LayerShape& shape : shapes) {
        ct_layer l;
        static_cast<LayerShape&>(l) = shape;
        if (l.d.kind == VPK_LAYER_CONV) {
            l.blob = blobs;
            counts[blobs++] = l.weights();
            counts[blobs++] = (size_t)l.OC;
        }
        s->L.push_back(l);
    }
    vpk_train_default_params(&s->ps.p);
    const hipError_t e = s->ps.alloc(counts, blobs);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        vpk_convtrain_free(h);
        return vpk_fail_hip(h, e, "vpk_convtrain_create: hipMalloc");
    }
    return VPK_OK;
}

int vpk_convtrain_destroy(vpk_handle* h) {
    if (!h) return VPK_ERR_ARG;
    vpk_convtrain_free(h);
    return VPK_OK;
}

int vpk_convtrain_set_params(vpk_handle* h, const vpk_train_params* p) {
    if (!h || !p) return VPK_ERR_ARG;
    if (!h->convtrain) return vpk_fail(h, VPK_ERR_STATE, "vpk_convtrain_set_params: no conv trainer (vpk_convtrain_create)");
    if (!stack_params_ok(*p)) return vpk_fail(h, VPK_ERR_ARG, "vpk_convtrain_set_params: stepsize must be >= 1");
    h->convtrain->ps.p = *p;
    return VPK_OK;
}

// a null list of blobs is looked at after the trainer, and only by a stack that has CONV layers (train_store.hpp)
int vpk_convtrain_load(vpk_handle* h, const void* const* blobs) {
    return vpk_store_load(h, store_of(h), "vpk_convtrain_load", blobs, false);
}

int vpk_convtrain_store(vpk_handle* h, void* const* blobs_out) {
    return vpk_store_copy(h, store_of(h), "vpk_convtrain_store", blobs_out, false, false, true, false);
}

int vpk_convtrain_load_momentum(vpk_handle* h, const void* const* blobs) {
    return vpk_store_copy(h, store_of(h), "vpk_convtrain_load_momentum", (void* const*)blobs, true, true, true, false);
}

int vpk_convtrain_store_momentum(vpk_handle* h, void* const* blobs_out) {
    return vpk_store_copy(h, store_of(h), "vpk_convtrain_store_momentum", blobs_out, true, false, true, false);
}

int vpk_convtrain_set_iteration(vpk_handle* h, long long iteration) {
    return vpk_store_set_iteration(h, store_of(h), "vpk_convtrain_set_iteration", iteration);
}

int vpk_convtrain_get_iteration(const vpk_handle* h, long long* iteration_out) {
    return vpk_store_get_iteration(store_of(h), iteration_out);
}

int vpk_convtrain_forward(vpk_handle* h, const float* X, int B, float* top_out) {
    if (!h) return VPK_ERR_ARG;
    vpk_convtrain_state* s = h->convtrain;
    if (!s || !s->ps.loaded) return vpk_fail(h, VPK_ERR_STATE, "vpk_convtrain_forward before vpk_convtrain_create / vpk_convtrain_load");
    if (B < 1 || B > CT_MAX_B) return vpk_fail(h, VPK_ERR_LIMIT, "vpk_convtrain_forward: the batch must be 1..32");
    if (!X) return vpk_fail(h, VPK_ERR_ARG, "vpk_convtrain_forward: X is required");
    VPK_HIP(h, hipSetDevice(h->device));
    if (int rc = reserve_blobs(h, s, B)) return rc;
    hipStream_t st = h->stream;
    s->kept.forward_begins();         // a refusal above leaves the kept blobs as they were, one below leaves none
    VPK_HIP(h, hipMemcpyAsync(s->xin, X, (size_t)B * s->in_size() * 4, hipMemcpyDeviceToDevice, st));
    const float* in = s->xin;
    for (ct_layer& L : s->L) {
        const vpk_stack_layer& d = L.d;
        if (d.kind == VPK_LAYER_CONV) {
            ct::ConvPtrs p = {in, s->ps.w[L.blob], s->ps.w[L.blob + 1], nullptr, nullptr, L.out};
            launch_gemm<ct::GEMM_FWD>(st, p, geom(L, B), 1, L.C / d.groups * d.kernel * d.kernel);
        } else if (d.kind == VPK_LAYER_LRN) {
            const Grid g = lrn_grid(L, B);
            ct_lrn_fwd<<<dim3(g.x, g.y), 256, lrn_lds_bytes(L), st>>>(in, L.out, L.scale, L.C, L.H * L.W, d.local_size,
                                                                      ct::lrn_alpha_over_n(d.alpha, d.local_size), d.beta, d.k);
        } else {
            const size_t planes = (size_t)B * L.C;
            ct_pool_fwd<<<blocks_of(planes * L.OH * L.OW), 256, 0, st>>>(in, L.out, L.idx, planes, L.H, L.W, L.OH, L.OW, d.kernel,
                                                                         d.stride);
        }
        in = L.out;
    }
    if (top_out)
        VPK_HIP(h, hipMemcpyAsync(top_out, s->L.back().out, blob_bytes(s->L.back(), B), hipMemcpyDeviceToDevice, st));
    VPK_HIP(h, hipGetLastError());
    s->kept.forward_done(B);
    return VPK_OK;
}

int vpk_convtrain_backward(vpk_handle* h, const float* d_top, float* d_input_out) {
    if (!h) return VPK_ERR_ARG;
    vpk_convtrain_state* s = h->convtrain;
    if (!s || !s->ps.loaded || !s->kept.backward_allowed())
        return vpk_fail(h, VPK_ERR_STATE, "vpk_convtrain_backward without a vpk_convtrain_forward to go back through");
    if (!d_top) return vpk_fail(h, VPK_ERR_ARG, "vpk_convtrain_backward: d_top is required");
    VPK_HIP(h, hipSetDevice(h->device));
    const int B = s->kept.fwd_B;
    hipStream_t st = h->stream;
    // the slabs of every weight gradient of this batch share one buffer
    if (const size_t want = slab_buffer_bytes(s->L, B))
        if (int rc = vpk_reserve(h, (void**)&s->partial, &s->partial_bytes, want, "vpk_convtrain_backward: weight-gradient slabs"))
            return rc;
    const Rates r = rates(s->ps.p, s->ps.iteration);
    const int n = (int)s->L.size();
    VPK_HIP(h, hipMemcpyAsync(s->L[n - 1].grad, d_top, blob_bytes(s->L[n - 1], B), hipMemcpyDeviceToDevice, st));
    for (int l = n - 1; l >= 0; --l) {
        ct_layer& L = s->L[l];
        const vpk_stack_layer& d = L.d;
        const float* in = l > 0 ? s->L[l - 1].out : s->xin;
        float* din = l > 0 ? s->L[l - 1].grad : d_input_out;        // NULL: the stack's input needs no gradient
        if (d.kind == VPK_LAYER_CONV) {
            const ct::ConvGeom q = geom(L, B);
            float *Wt = s->ps.w[L.blob], *bias = s->ps.w[L.blob + 1];
            if (din) {
                ct::ConvPtrs p = {in, Wt, bias, L.out, L.grad, din};
                launch_gemm<ct::GEMM_DGRAD>(st, p, q, 1, q.OCg() * q.K * q.K);
            }
            const WgradPlan wg = plan_wgrad(L, B);
            ct::ConvPtrs p = {in, Wt, bias, L.out, L.grad, s->partial};
            launch_gemm<ct::GEMM_WGRAD>(st, p, q, wg.slabs, wg.slab_len);
            ct_update<<<blocks_of((size_t)L.OC * wg.cols), 256, 0, st>>>(Wt, s->ps.v[L.blob], bias, s->ps.v[L.blob + 1], s->partial,
                                                                         wg.slabs, L.OC, wg.cols, r.lr_w, r.dec_w, r.lr_b, r.dec_b,
                                                                         r.mu);
        } else if (!din) {
            continue;
        } else if (d.kind == VPK_LAYER_LRN) {
            const Grid g = lrn_grid(L, B);
            ct_lrn_bwd<<<dim3(g.x, g.y), 256, lrn_lds_bytes(L), st>>>(in, L.out, L.scale, L.grad, din, L.C, L.H * L.W, d.local_size,
                                                                      d.beta, ct::lrn_back_coef(d.alpha, d.beta, d.local_size));
        } else {
            const size_t planes = (size_t)B * L.C;
            ct_pool_bwd<<<blocks_of(planes * L.H * L.W), 256, 0, st>>>(L.grad, L.idx, din, planes, L.H, L.W, L.OH, L.OW, d.kernel,
                                                                       d.stride);
        }
    }
    VPK_HIP(h, hipGetLastError());
    s->kept.backward_done();
    s->ps.iteration += 1;
    return VPK_OK;
}

int vpk_convtrain_read(vpk_handle* h, int layer, int kind, void* out) {
    if (!h) return VPK_ERR_ARG;
    vpk_convtrain_state* s = h->convtrain;
    if (!s || !s->kept.read_allowed()) return vpk_fail(h, VPK_ERR_STATE, "vpk_convtrain_read without a forward");
    if (!out) return vpk_fail(h, VPK_ERR_ARG, "vpk_convtrain_read: out is required");
    if (layer < 0 || layer >= (int)s->L.size()) return vpk_fail(h, VPK_ERR_ARG, "vpk_convtrain_read: no such layer");
    const ct_layer& L = s->L[layer];
    const void* src = nullptr;
    if (kind == VPK_BLOB_OUTPUT) src = L.out;
    else if (kind == VPK_BLOB_POOL_INDEX) {
        if (L.d.kind != VPK_LAYER_POOL) return vpk_fail(h, VPK_ERR_ARG, "vpk_convtrain_read: not a POOL layer");
        src = L.idx;
    } else if (kind == VPK_BLOB_LRN_SCALE) {
        if (L.d.kind != VPK_LAYER_LRN) return vpk_fail(h, VPK_ERR_ARG, "vpk_convtrain_read: not an LRN layer");
        src = L.scale;
    } else if (kind == VPK_BLOB_GRADIENT) {
        if (!s->kept.gradient_read_allowed()) return vpk_fail(h, VPK_ERR_STATE, "vpk_convtrain_read: no backward since the last forward");
        src = L.grad;
    } else {
        return vpk_fail(h, VPK_ERR_ARG, "vpk_convtrain_read: unknown kind");
    }
    VPK_HIP(h, hipSetDevice(h->device));
    VPK_HIP(h, hipMemcpyAsync(out, src, blob_bytes(L, s->kept.blob_B), hipMemcpyDeviceToDevice, h->stream));
    return VPK_OK;
}

}  // extern "C"
