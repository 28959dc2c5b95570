// vpk_train.hip -- SGD fine-tuning of the net's dense head (fc6, fc7, fc8) on float32 master weights.
//
// One step (train/train_val.prototxt:289-417 under train/solver.prototxt) is
//   forward   three skinny products, each ONE read of its W, K split into slabs      (train_fwd, train_fwd_finish)
//   loss      sigmoid cross-entropy, its gradient and the sigmoid output             (train_loss)
//   backward  per layer ONE sweep over W and V: the tile of dW is formed in registers from the staged dY and X, the tile's
//             share of dX is taken from the old W, and the new V and W are written in place                (train_sweep)
//             dX: per-row-tile partial sums, added in tile order with the dropout/ReLU backward applied    (train_dx_reduce)
// No dW buffer exists and no float atomic is used: two runs from the same state give the same bits.
// Arithmetic: f32 parameters, f32 accumulation, VALU FMAs.  The per-element functions are train_device.hpp's.
// What the host decides lives elsewhere: the tile constants, the launch plans, the workspace sizes, the solver's rates and
// the set_params rule in train_plan.hpp (host-tested); the weights, momentum, iteration and their load / store entry points
// in train_store.hpp, shared with vpk_convtrain.hip.  Here are the kernels, the launches and the step's own refusals.
#include "vpk_internal.hpp"
#include "train_device.hpp"
#include "train_plan.hpp"
#include "train_store.hpp"

#include <string.h>

using namespace vpk_train_plan;

namespace {

// 4 consecutive floats of a row from column k.  VEC: the row is 16-byte aligned and K % 4 == 0, so a group is wholly inside
// the row or wholly outside; otherwise element by element.  Outside the row: zeros.
template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* __restrict__ row, int k, int K) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {
        if (k < K) r = *reinterpret_cast<const float4*>(row + k);
    } else {
        if (k < K) r.x = row[k];
        if (k + 1 < K) r.y = row[k + 1];
        if (k + 2 < K) r.z = row[k + 2];
        if (k + 3 < K) r.w = row[k + 3];
    }
    return r;
}

template <bool VEC>
__device__ __forceinline__ void st4(float* __restrict__ row, int k, int K, float4 v) {
    if (VEC) {
        if (k < K) *reinterpret_cast<float4*>(row + k) = v;
    } else {
        if (k < K) row[k] = v.x;
        if (k + 1 < K) row[k + 1] = v.y;
        if (k + 2 < K) row[k + 2] = v.z;
        if (k + 3 < K) row[k + 3] = v.w;
    }
}

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);     // a fixed butterfly: every lane ends with the same sum
    return v;
}

// The forward's sweep: a workgroup owns FWD_RT rows of W (4 per wave) and a slab of 256-column chunks.  Per chunk the lanes
// load their 4 rows x 4 columns of W, the workgroup stages the chunk of X in LDS once for its four waves, and each lane
// accumulates its columns' share of Y[b][n] for every b.  The lanes are then added by a fixed butterfly and the slab's
// sums stored: partial[slab][b][n].  train_fwd_finish adds the slabs in slab order.
template <int NB, bool VEC>
__global__ __launch_bounds__(256) void train_fwd(const float* __restrict__ W, const float* __restrict__ X, int B, int N, int K,
                                                 int chunks, int chunks_per_slab, float* __restrict__ partial) {
    __shared__ float4 xs[NB][64];
    __shared__ float red[FWD_RT][NB];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nblk = blockIdx.y * FWD_RT, n0 = nblk + wave * FWD_ROWS;
    const int c0 = blockIdx.x * chunks_per_slab, c1 = min(c0 + chunks_per_slab, chunks);
    float acc[FWD_ROWS][NB];
#pragma unroll
    for (int r = 0; r < FWD_ROWS; ++r)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[r][b] = 0.f;
    const float* rows[FWD_ROWS];
#pragma unroll
    for (int r = 0; r < FWD_ROWS; ++r) rows[r] = W + (size_t)min(n0 + r, N - 1) * K;     // rows past N: computed, not stored
    // the next chunk's W and X are loaded into registers while this chunk is worked on
    constexpr int XS = NB * 64 / 256;                                // float4 of the X chunk each thread stages
    float4 wn[FWD_ROWS], xn[XS];
    auto load_chunk = [&](int c) {
        const int k0 = c * SWEEP_KT;
#pragma unroll
        for (int r = 0; r < FWD_ROWS; ++r) wn[r] = ld4<VEC>(rows[r], k0 + lane * 4, K);
#pragma unroll
        for (int j = 0; j < XS; ++j) {
            const int b = wave + 4 * j;                              // thread (wave, lane) stages xs[wave + 4 j][lane]
            xn[j] = b < B ? ld4<VEC>(X + (size_t)b * K, k0 + lane * 4, K) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    if (c0 < c1) load_chunk(c0);
    for (int c = c0; c < c1; ++c) {
        float4 w[FWD_ROWS];
#pragma unroll
        for (int r = 0; r < FWD_ROWS; ++r) w[r] = wn[r];
#pragma unroll
        for (int j = 0; j < XS; ++j) xs[wave + 4 * j][lane] = xn[j];
        __syncthreads();
        if (c + 1 < c1) load_chunk(c + 1);
        // groups of 8 images under one wave-uniform test (rows b >= B of xs are zero): long enough for the LDS reads to pipeline
#pragma unroll
        for (int g = 0; g < NB; g += 8) {
            if (g < B) {
#pragma unroll
                for (int b = g; b < g + 8; ++b) {
                    const float4 x = xs[b][lane];
#pragma unroll
                    for (int r = 0; r < FWD_ROWS; ++r)
                        acc[r][b] += w[r].x * x.x + w[r].y * x.y + w[r].z * x.z + w[r].w * x.w;
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < FWD_ROWS; ++r)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float s = wave_sum(acc[r][b]);
            if (lane == 0) red[wave * FWD_ROWS + r][b] = s;
        }
    __syncthreads();
    float* dst = partial + (size_t)blockIdx.x * B * N;
    for (int i = threadIdx.x; i < FWD_RT * NB; i += 256) {
        const int r = i % FWD_RT, b = i / FWD_RT, n = nblk + r;
        if (n < N && b < B) dst[(size_t)b * N + n] = red[r][b];
    }
}

// Y = sum of the slabs in slab order + bias.  relu: A = max(Y, 0), else A = Y.  D (optional) = A * mask * scale (mask null: A).
__global__ void train_fwd_finish(const float* __restrict__ partial, int slabs, int B, int N, const float* __restrict__ bias,
                                 float* __restrict__ A, float* __restrict__ D, const uint8_t* __restrict__ mask, float scale,
                                 int relu) {
    const size_t BN = (size_t)B * N, o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= BN) return;
    float y = 0.f;
#pragma unroll 8
    for (int t = 0; t < slabs; ++t) y += partial[(size_t)t * BN + o];
    y += bias[o % N];
    if (relu) y = fmaxf(y, 0.f);
    A[o] = y;
    if (D) D[o] = mask ? y * ((float)mask[o] * scale) : y;
}

// The fused backward and update of one layer Y = Xin W^T: a workgroup owns rows [n0, n0 + RT) x columns [k0, k0 + 256) of W
// and V.  Each wave takes every fourth row; a lane owns 4 columns.  Per row: dW = sum_b dY[b][n] Xin[b][k] in registers,
// dX[b][k] += dY[b][n] W_old[n][k] (DX only), then Caffe's update of the 4 elements, stored in place.  The four waves' dX
// are added in wave order through LDS and written as this row tile's partial: partial[tile][b][k].
template <int NB, bool VEC, bool DX>
__global__ __launch_bounds__(256) void train_sweep(float* __restrict__ W, float* __restrict__ V, const float* __restrict__ dY,
                                                   const float* __restrict__ Xin, int B, int N, int K, int RT,
                                                   float* __restrict__ partial, float lr, float decay, float mu) {
    __shared__ float4 xs[NB][64];
    __shared__ float dys[SWEEP_MAX_RT][NB];
    const int k0 = blockIdx.x * SWEEP_KT;
    const int n0 = blockIdx.y * RT, n1 = min(n0 + RT, N);
    for (int i = threadIdx.x; i < NB * 64; i += 256) {
        const int b = i >> 6, l = i & 63;
        xs[b][l] = b < B ? ld4<VEC>(Xin + (size_t)b * K, k0 + l * 4, K) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int i = threadIdx.x; i < RT * NB; i += 256) {
        const int r = i / NB, b = i % NB, n = n0 + r;
        dys[r][b] = (b < B && n < n1) ? dY[(size_t)b * N + n] : 0.f;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = k0 + lane * 4;
    float4 dx[DX ? NB : 1];
#pragma unroll
    for (int b = 0; b < (DX ? NB : 1); ++b) dx[b] = make_float4(0.f, 0.f, 0.f, 0.f);
    // two rows in flight per wave: the loads of the second are issued before the first is worked on
    for (int n = n0 + wave; n < n1; n += 8) {
        const int nb = n + 4;
        const bool two = nb < n1;                                    // the same in every lane of the wave
        float* wr0 = W + (size_t)n * K;
        float* vr0 = V + (size_t)n * K;
        float* wr1 = W + (size_t)(two ? nb : n) * K;
        float* vr1 = V + (size_t)(two ? nb : n) * K;
        float4 w0 = ld4<VEC>(wr0, k, K), v0 = ld4<VEC>(vr0, k, K);
        float4 w1 = ld4<VEC>(wr1, k, K), v1 = ld4<VEC>(vr1, k, K);
        float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;
        const int r0 = n - n0, r1 = (two ? nb : n) - n0;
        // groups of 8 images under one wave-uniform test (rows b >= B of xs and dys are zero)
#pragma unroll
        for (int g = 0; g < NB; g += 8) {
            if (g < B) {
#pragma unroll
                for (int b = g; b < g + 8; ++b) {
                    const float4 x = xs[b][lane];
                    const float y0 = dys[r0][b], y1 = two ? dys[r1][b] : 0.f;
                    g0.x += y0 * x.x; g0.y += y0 * x.y; g0.z += y0 * x.z; g0.w += y0 * x.w;
                    g1.x += y1 * x.x; g1.y += y1 * x.y; g1.z += y1 * x.z; g1.w += y1 * x.w;
                    if (DX) {
                        dx[b].x += y0 * w0.x; dx[b].y += y0 * w0.y; dx[b].z += y0 * w0.z; dx[b].w += y0 * w0.w;
                        dx[b].x += y1 * w1.x; dx[b].y += y1 * w1.y; dx[b].z += y1 * w1.z; dx[b].w += y1 * w1.w;
                    }
                }
            }
        }
        vpk_train::sgd_update(w0.x, v0.x, g0.x, lr, decay, mu);
        vpk_train::sgd_update(w0.y, v0.y, g0.y, lr, decay, mu);
        vpk_train::sgd_update(w0.z, v0.z, g0.z, lr, decay, mu);
        vpk_train::sgd_update(w0.w, v0.w, g0.w, lr, decay, mu);
        st4<VEC>(wr0, k, K, w0);
        st4<VEC>(vr0, k, K, v0);
        if (two) {
            vpk_train::sgd_update(w1.x, v1.x, g1.x, lr, decay, mu);
            vpk_train::sgd_update(w1.y, v1.y, g1.y, lr, decay, mu);
            vpk_train::sgd_update(w1.z, v1.z, g1.z, lr, decay, mu);
            vpk_train::sgd_update(w1.w, v1.w, g1.w, lr, decay, mu);
            st4<VEC>(wr1, k, K, w1);
            st4<VEC>(vr1, k, K, v1);
        }
    }
    if (DX) {
        __syncthreads();                                             // every wave is done reading xs
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (b < B) {
                        float4 s = dx[b];
                        if (w > 0) {
                            const float4 p = xs[b][lane];
                            s.x = p.x + s.x; s.y = p.y + s.y; s.z = p.z + s.z; s.w = p.w + s.w;
                        }
                        xs[b][lane] = s;
                    }
                }
            }
            __syncthreads();
        }
        float* dst = partial + (size_t)blockIdx.y * B * K;
        for (int i = threadIdx.x; i < B * 64; i += 256) {
            const int b = i >> 6, l = i & 63;
            st4<VEC>(dst + (size_t)b * K, k0 + l * 4, K, xs[b][l]);
        }
    }
}

// dX[b][k] = sum over the row tiles, in tile order; then through dropout and ReLU: dA = dX * mask * scale * [act > 0]
__global__ void train_dx_reduce(const float* __restrict__ partial, int tiles, size_t BK, const uint8_t* __restrict__ mask,
                                const float* __restrict__ act, float scale, float* __restrict__ dA) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BK) return;
    float s = 0.f;
#pragma unroll 8
    for (int t = 0; t < tiles; ++t) s += partial[(size_t)t * BK + i];       // (the loads of 8 tiles in flight, the adds in order)
    dA[i] = act[i] > 0.f ? s * ((float)mask[i] * scale) : 0.f;
}

// dX[b][k] = sum over the row tiles, in tile order, as it is (vpk_train_step_dx: the gradient that leaves the head)
__global__ void train_dx_sum(const float* __restrict__ partial, int tiles, size_t BK, float* __restrict__ dX) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BK) return;
    float s = 0.f;
#pragma unroll 8
    for (int t = 0; t < tiles; ++t) s += partial[(size_t)t * BK + i];
    dX[i] = s;
}

// db[n] = sum_b dY[b][n] in batch order, and the bias's update (lr_mult 2, decay_mult 0 come in through lr and decay)
__global__ void train_bias(float* __restrict__ bias, float* __restrict__ vb, const float* __restrict__ dY, int B, int N,
                           float lr, float decay, float mu) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float g = 0.f;
    for (int b = 0; b < B; ++b) g += dY[(size_t)b * N + n];
    float w = bias[n], v = vb[n];
    vpk_train::sgd_update(w, v, g, lr, decay, mu);
    bias[n] = w;
    vb[n] = v;
}

// one workgroup: sigout, dz (training only) and the loss of count = B x O logits, summed in a fixed tree;
// *loss_out = (accumulate ? *loss_out : 0) + sum * inv_b.  t null: sigout only.
__global__ __launch_bounds__(256) void train_loss(const float* __restrict__ z, const float* __restrict__ t, int count,
                                                  float inv_b, float* __restrict__ sig, float* __restrict__ dz,
                                                  float* __restrict__ loss_out, int accumulate) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < count; i += 256) {
        const float zi = z[i];
        if (sig) sig[i] = vpk_train::sigmoid(zi);
        if (t) {
            const float ti = t[i];
            s += vpk_train::loss_term(zi, ti);
            if (dz) dz[i] = vpk_train::loss_grad(zi, ti, inv_b);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && loss_out && t) *loss_out = (accumulate ? *loss_out : 0.f) + red[0] * inv_b;
}

__global__ void train_masks(uint8_t* __restrict__ m, int B, int H, uint64_t seed, uint64_t iteration, uint32_t layer,
                            uint32_t threshold) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * H) return;
    const uint32_t b = (uint32_t)(i / H), j = (uint32_t)(i % H);
    m[i] = vpk_train::mask_bit(vpk_train::mask_key(seed, iteration, layer, b), j, threshold);
}

}  // namespace

struct vpk_train_state {
    int dims[4] = {};                 // I, H6, H7, O
    vpk_param_store ps;               // fc6 [H6 x I], its bias, fc7 [H7 x H6], its bias, fc8 [O x H7], its bias; their momentum
    float *a6 = nullptr, *d6 = nullptr, *a7 = nullptr, *d7 = nullptr;       // TRAIN_MAX_B rows each
    float *z = nullptr, *dz = nullptr, *sig = nullptr, *dA7 = nullptr, *dA6 = nullptr;
    uint8_t *m6 = nullptr, *m7 = nullptr;
    float* partial = nullptr;         // the sweeps' dX partials: [row tile][B][K]
    float* fpartial = nullptr;        // the forward's slab sums: [slab][B][N]
    float* xpartial = nullptr;        // fc6's dX partials [row tile][B][I]: vpk_train_step_dx only, allocated by its first call
    size_t xpartial_bytes = 0;
    float* W(int l) const { return ps.w[2 * l]; }
    float* V(int l) const { return ps.v[2 * l]; }
    float* b(int l) const { return ps.w[2 * l + 1]; }
    float* vb(int l) const { return ps.v[2 * l + 1]; }
};

namespace {

vpk_param_store* store_of(const vpk_handle* h) { return h && h->train ? &h->train->ps : nullptr; }

template <int NB>
void launch_fwd(hipStream_t st, bool vec, const FwdPlan& p, const float* W, const float* X, int B, int N, int K, float* partial) {
    const dim3 grid(p.slabs, p.row_tiles);
    if (vec) train_fwd<NB, true><<<grid, 256, 0, st>>>(W, X, B, N, K, p.chunks, p.chunks_per_slab, partial);
    else train_fwd<NB, false><<<grid, 256, 0, st>>>(W, X, B, N, K, p.chunks, p.chunks_per_slab, partial);
}

void forward_layer(hipStream_t st, const float* W, const float* bias, const float* X, int B, int N, int K, float* partial,
                   float* A, float* D, const uint8_t* mask, float scale, int relu) {
    const bool vec = vec_ok(K, {W, X});
    const FwdPlan p = plan_fwd(N, K);
    if (batch_nb(B) == 8) launch_fwd<8>(st, vec, p, W, X, B, N, K, partial);
    else launch_fwd<TRAIN_MAX_B>(st, vec, p, W, X, B, N, K, partial);
    train_fwd_finish<<<blocks_of((size_t)B * N), 256, 0, st>>>(partial, p.slabs, B, N, bias, A, D, mask, scale, relu);
}

template <int NB, bool DX>
void launch_sweep(hipStream_t st, bool vec, float* W, float* V, const float* dY, const float* Xin, int B, int N, int K,
                  float* partial, float lr, float decay, float mu) {
    const SweepPlan p = plan_sweep(N, K);
    const dim3 grid(p.col_tiles, p.tiles);
    if (vec) train_sweep<NB, true, DX><<<grid, 256, 0, st>>>(W, V, dY, Xin, B, N, K, p.rt, partial, lr, decay, mu);
    else train_sweep<NB, false, DX><<<grid, 256, 0, st>>>(W, V, dY, Xin, B, N, K, p.rt, partial, lr, decay, mu);
}

// partial null: the sweep without its dX
void sweep_layer(hipStream_t st, float* W, float* V, const float* dY, const float* Xin, int B, int N, int K, float* partial,
                 float lr, float decay, float mu) {
    const bool vec = vec_ok(K, {W, V, Xin, partial});
    if (partial) {
        if (batch_nb(B) == 8) launch_sweep<8, true>(st, vec, W, V, dY, Xin, B, N, K, partial, lr, decay, mu);
        else launch_sweep<TRAIN_MAX_B, true>(st, vec, W, V, dY, Xin, B, N, K, partial, lr, decay, mu);
    } else {
        if (batch_nb(B) == 8) launch_sweep<8, false>(st, vec, W, V, dY, Xin, B, N, K, nullptr, lr, decay, mu);
        else launch_sweep<TRAIN_MAX_B, false>(st, vec, W, V, dY, Xin, B, N, K, nullptr, lr, decay, mu);
    }
}

// the forward of B <= TRAIN_MAX_B rows into the state's activations; training: with the masks in s->m6 / s->m7
void forward(vpk_handle* h, vpk_train_state* s, const float* X, int B, bool training) {
    const int I = s->dims[0], H6 = s->dims[1], H7 = s->dims[2], O = s->dims[3];
    const float scale = training ? 1.0f / (1.0f - s->ps.p.dropout_ratio) : 1.0f;
    forward_layer(h->stream, s->W(0), s->b(0), X, B, H6, I, s->fpartial, s->a6, s->d6, training ? s->m6 : nullptr, scale, 1);
    forward_layer(h->stream, s->W(1), s->b(1), s->d6, B, H7, H6, s->fpartial, s->a7, s->d7, training ? s->m7 : nullptr, scale, 1);
    forward_layer(h->stream, s->W(2), s->b(2), s->d7, B, O, H7, s->fpartial, s->z, nullptr, nullptr, 1.0f, 0);
}

}  // namespace

void vpk_train_free(vpk_handle* h) {
    vpk_train_state* s = h->train;
    if (!s) return;
    (void)hipStreamSynchronize(h->stream);
    s->ps.free();
    for (void* p : {(void*)s->a6, (void*)s->d6, (void*)s->a7, (void*)s->d7, (void*)s->z, (void*)s->dz, (void*)s->sig,
                    (void*)s->dA7, (void*)s->dA6, (void*)s->m6, (void*)s->m7, (void*)s->partial, (void*)s->fpartial,
                    (void*)s->xpartial})
        if (p) (void)hipFree(p);
    delete s;
    h->train = nullptr;
}

extern "C" {

void vpk_train_default_params(vpk_train_params* p) {
    if (!p) return;
    p->base_lr = 1e-4f;           // solver.prototxt:8
    p->gamma = 0.1f;              // :10
    p->stepsize = 200000;         // :11
    p->momentum = 0.9f;           // :17
    p->weight_decay = 5e-4f;      // :18
    p->lr_mult_weight = 1.0f;     // train_val.prototxt:295, 335, 375
    p->decay_mult_weight = 1.0f;  // :296, 336, 376
    p->lr_mult_bias = 2.0f;       // :299, 339, 379
    p->decay_mult_bias = 0.0f;    // :300, 340, 380
    p->dropout_ratio = 0.5f;      // :326, 366
}

int vpk_train_create(vpk_handle* h, const int32_t dims[4]) {
    if (!h || !dims) return VPK_ERR_ARG;
    for (int i = 0; i < 4; ++i)
        if (dims[i] < 1) return vpk_fail(h, VPK_ERR_ARG, "vpk_train_create: sizes must be positive");
    if (h->train) return vpk_fail(h, VPK_ERR_STATE, "vpk_train_create: the handle already has a trainer");
    VPK_HIP(h, hipSetDevice(h->device));
    vpk_train_state* s = new vpk_train_state();
    h->train = s;
    for (int i = 0; i < 4; ++i) s->dims[i] = dims[i];
    vpk_train_default_params(&s->ps.p);
    const size_t mb = TRAIN_MAX_B, I = dims[0], H6 = dims[1], H7 = dims[2], O = dims[3];
    const size_t counts[6] = {H6 * I, H6, H7 * H6, H7, O * H7, O};
    hipError_t e = s->ps.alloc(counts, 6);
    auto alloc = [&](void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    alloc((void**)&s->a6, mb * H6 * 4);
    alloc((void**)&s->d6, mb * H6 * 4);
    alloc((void**)&s->dA6, mb * H6 * 4);
    alloc((void**)&s->m6, mb * H6);
    alloc((void**)&s->a7, mb * H7 * 4);
    alloc((void**)&s->d7, mb * H7 * 4);
    alloc((void**)&s->dA7, mb * H7 * 4);
    alloc((void**)&s->m7, mb * H7);
    alloc((void**)&s->z, mb * O * 4);
    alloc((void**)&s->dz, mb * O * 4);
    alloc((void**)&s->sig, mb * O * 4);
    alloc((void**)&s->partial, partial_bytes(s->dims));
    alloc((void**)&s->fpartial, fpartial_bytes(s->dims));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        vpk_train_free(h);
        return vpk_fail_hip(h, e, "vpk_train_create: hipMalloc");
    }
    return VPK_OK;
}

int vpk_train_destroy(vpk_handle* h) {
    if (!h) return VPK_ERR_ARG;
    vpk_train_free(h);
    return VPK_OK;
}

int vpk_train_set_params(vpk_handle* h, const vpk_train_params* p) {
    if (!h || !p) return VPK_ERR_ARG;
    if (!h->train) return vpk_fail(h, VPK_ERR_STATE, "vpk_train_set_params: no trainer (vpk_train_create)");
    if (!head_params_ok(*p))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_train_set_params: dropout_ratio must be in [0, 1) and stepsize >= 1");
    h->train->ps.p = *p;
    return VPK_OK;
}

// a null list of blobs is VPK_ERR_ARG without a message, before anything else is looked at (train_store.hpp: silent_null)
int vpk_train_load(vpk_handle* h, const void* const blobs[6]) {
    return vpk_store_load(h, store_of(h), "vpk_train_load", blobs, true);
}

int vpk_train_store(vpk_handle* h, void* const blobs_out[6]) {
    return vpk_store_copy(h, store_of(h), "vpk_train_store", blobs_out, false, false, true, true);
}

int vpk_train_load_momentum(vpk_handle* h, const void* const blobs[6]) {
    return vpk_store_copy(h, store_of(h), "vpk_train_load_momentum", (void* const*)blobs, true, true, true, true);
}

int vpk_train_store_momentum(vpk_handle* h, void* const blobs_out[6]) {
    return vpk_store_copy(h, store_of(h), "vpk_train_store_momentum", blobs_out, true, false, true, true);
}

int vpk_train_set_iteration(vpk_handle* h, long long iteration) {
    return vpk_store_set_iteration(h, store_of(h), "vpk_train_set_iteration", iteration);
}

int vpk_train_get_iteration(const vpk_handle* h, long long* iteration_out) {
    return vpk_store_get_iteration(store_of(h), iteration_out);
}

// the step; want_dx: vpk_train_step_dx, which also writes dX_out (the fc6 sweep's DX form and its partials)
static int train_step(vpk_handle* h, const float* X, const float* labels, int B, const uint8_t* mask6, const uint8_t* mask7,
                      unsigned long long seed, float* loss_out, float* sigout_out, bool want_dx, float* dX_out) {
    if (!h) return VPK_ERR_ARG;
    vpk_train_state* s = h->train;
    if (!s || !s->ps.loaded) return vpk_fail(h, VPK_ERR_STATE, "vpk_train_step before vpk_train_create / vpk_train_load");
    if (B < 1 || B > TRAIN_MAX_B) return vpk_fail(h, VPK_ERR_LIMIT, "vpk_train_step: the batch must be 1..32");
    if (!X || !labels || (mask6 == nullptr) != (mask7 == nullptr) || (want_dx && !dX_out))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_train_step: X, labels (and dX_out) are required, the masks come both or not at all");
    VPK_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const int I = s->dims[0], H6 = s->dims[1], H7 = s->dims[2], O = s->dims[3];
    if (want_dx) {
        const int rc = vpk_reserve(h, (void**)&s->xpartial, &s->xpartial_bytes, xpartial_bytes(s->dims, B),
                                   "vpk_train_step_dx: fc6 dX partials");
        if (rc) return rc;
    }
    const vpk_train_params& p = s->ps.p;
    const long long iteration = s->ps.iteration;
    if (mask6) {
        VPK_HIP(h, hipMemcpyAsync(s->m6, mask6, (size_t)B * H6, hipMemcpyDeviceToDevice, st));
        VPK_HIP(h, hipMemcpyAsync(s->m7, mask7, (size_t)B * H7, hipMemcpyDeviceToDevice, st));
    } else {
        const uint32_t thr = vpk_train::mask_threshold(p.dropout_ratio);
        train_masks<<<blocks_of((size_t)B * H6), 256, 0, st>>>(s->m6, B, H6, seed, (uint64_t)iteration, 6u, thr);
        train_masks<<<blocks_of((size_t)B * H7), 256, 0, st>>>(s->m7, B, H7, seed, (uint64_t)iteration, 7u, thr);
    }
    forward(h, s, X, B, true);
    float* sig = sigout_out ? sigout_out : s->sig;
    train_loss<<<1, 256, 0, st>>>(s->z, labels, B * O, 1.0f / (float)B, sig, s->dz, loss_out, 0);

    const Rates r = rates(p, iteration);
    const float scale = 1.0f / (1.0f - p.dropout_ratio);
    // fc8: dY = dz, input d7; its dX goes back through drop7 and relu7
    sweep_layer(st, s->W(2), s->V(2), s->dz, s->d7, B, O, H7, s->partial, r.lr_w, r.dec_w, r.mu);
    train_bias<<<blocks_of(O), 256, 0, st>>>(s->b(2), s->vb(2), s->dz, B, O, r.lr_b, r.dec_b, r.mu);
    const size_t bk7 = (size_t)B * H7, bk6 = (size_t)B * H6;
    train_dx_reduce<<<blocks_of(bk7), 256, 0, st>>>(s->partial, plan_sweep(O, H7).tiles, bk7, s->m7, s->a7, scale, s->dA7);
    // fc7
    sweep_layer(st, s->W(1), s->V(1), s->dA7, s->d6, B, H7, H6, s->partial, r.lr_w, r.dec_w, r.mu);
    train_bias<<<blocks_of(H7), 256, 0, st>>>(s->b(1), s->vb(1), s->dA7, B, H7, r.lr_b, r.dec_b, r.mu);
    train_dx_reduce<<<blocks_of(bk6), 256, 0, st>>>(s->partial, plan_sweep(H7, H6).tiles, bk6, s->m6, s->a6, scale, s->dA6);
    // fc6: no dX while the conv stack below is frozen (vpk_train_step); vpk_train_step_dx hands it to the caller
    sweep_layer(st, s->W(0), s->V(0), s->dA6, X, B, H6, I, want_dx ? s->xpartial : nullptr, r.lr_w, r.dec_w, r.mu);
    if (want_dx)
        train_dx_sum<<<blocks_of((size_t)B * I), 256, 0, st>>>(s->xpartial, plan_sweep(H6, I).tiles, (size_t)B * I, dX_out);
    train_bias<<<blocks_of(H6), 256, 0, st>>>(s->b(0), s->vb(0), s->dA6, B, H6, r.lr_b, r.dec_b, r.mu);
    VPK_HIP(h, hipGetLastError());
    s->ps.iteration += 1;
    return VPK_OK;
}

int vpk_train_step(vpk_handle* h, const float* X, const float* labels, int B, const uint8_t* mask6, const uint8_t* mask7,
                   unsigned long long seed, float* loss_out, float* sigout_out) {
    return train_step(h, X, labels, B, mask6, mask7, seed, loss_out, sigout_out, false, nullptr);
}

int vpk_train_step_dx(vpk_handle* h, const float* X, const float* labels, int B, const uint8_t* mask6, const uint8_t* mask7,
                      unsigned long long seed, float* loss_out, float* sigout_out, float* dX_out) {
    return train_step(h, X, labels, B, mask6, mask7, seed, loss_out, sigout_out, true, dX_out);
}

int vpk_train_eval(vpk_handle* h, const float* X, const float* labels, int B, float* loss_out, float* sigout_out) {
    if (!h) return VPK_ERR_ARG;
    vpk_train_state* s = h->train;
    if (!s || !s->ps.loaded) return vpk_fail(h, VPK_ERR_STATE, "vpk_train_eval before vpk_train_create / vpk_train_load");
    if (B < 1 || !X || (labels && !loss_out)) return vpk_fail(h, VPK_ERR_ARG, "vpk_train_eval: B >= 1, X, and loss_out with labels");
    VPK_HIP(h, hipSetDevice(h->device));
    const int I = s->dims[0], O = s->dims[3];
    const float inv_b = 1.0f / (float)B;
    for (int b0 = 0; b0 < B; b0 += TRAIN_MAX_B) {
        const int nb = B - b0 < TRAIN_MAX_B ? B - b0 : TRAIN_MAX_B;
        forward(h, s, X + (size_t)b0 * I, nb, false);
        float* sig = sigout_out ? sigout_out + (size_t)b0 * O : s->sig;
        train_loss<<<1, 256, 0, h->stream>>>(s->z, labels ? labels + (size_t)b0 * O : nullptr, nb * O, inv_b, sig, nullptr,
                                              loss_out, b0 > 0);
    }
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // extern "C"
