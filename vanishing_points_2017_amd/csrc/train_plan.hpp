// train_plan.hpp -- what the two training drivers (vpk_train.hip, vpk_convtrain.hip) decide on the host: the head's launch
// plans and workspace sizes, the conv stack's shapes, limits, grids and buffer sizes, the life cycle of the stack's kept
// blobs, the solver's rates of an iteration and the two set_params validators.  Pure functions of their arguments; no HIP
// type and no HIP include: tests/hostsim/sim_train_plan.cpp compiles it with g++ for the CPU tests (tests/test_train_plan.py).
// The constants are the kernels' too, which use them by name.
#ifndef VPK_TRAIN_PLAN_HPP_
#define VPK_TRAIN_PLAN_HPP_

#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <vector>

#include "../../include/vpk.h"
#include "convtrain_device.hpp"
#include "train_device.hpp"

#pragma GCC visibility push(hidden)   // host helpers of the units that include this: nothing here is an export
namespace vpk_train_plan {

// ---- the dense head -----------------------------------------------------------------------------------------------------
constexpr int TRAIN_MAX_B = 32;       // rows of a step: dY and X of a tile stay in LDS, the dX accumulators in registers
constexpr int FWD_ROWS = 4;           // rows of W per forward wave
constexpr int FWD_RT = 16;            // ... and per workgroup of four waves
constexpr int SWEEP_KT = 256;         // columns of a sweep tile: 64 lanes x 4
constexpr int SWEEP_MAX_RT = 128;     // most rows of a sweep tile (its dY slice is staged in LDS)
constexpr int SWEEP_MIN_RT = 16;
constexpr int SWEEP_TARGET_BLOCKS = 2048;

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// the backward's sweep over an N x K layer: rows of a tile -- as many as keep about SWEEP_TARGET_BLOCKS workgroups, a
// multiple of 8 within the LDS slice -- and the grid (col_tiles, tiles)
struct SweepPlan { int rt, tiles, col_tiles; };
inline SweepPlan plan_sweep(int N, int K) {
    const long long kt = ceil_div(K, SWEEP_KT);
    long long rt = ((long long)N * kt + SWEEP_TARGET_BLOCKS - 1) / SWEEP_TARGET_BLOCKS;
    rt = (rt + 7) / 8 * 8;
    if (rt < SWEEP_MIN_RT) rt = SWEEP_MIN_RT;
    if (rt > SWEEP_MAX_RT) rt = SWEEP_MAX_RT;
    return SweepPlan{(int)rt, ceil_div(N, (int)rt), (int)kt};
}

// the forward's split of K: 256-column chunks, dealt to as many slabs as keep about SWEEP_TARGET_BLOCKS workgroups;
// grid (slabs, row_tiles)
struct FwdPlan { int chunks, chunks_per_slab, slabs, row_tiles; };
inline FwdPlan plan_fwd(int N, int K) {
    FwdPlan p;
    p.chunks = ceil_div(K, SWEEP_KT);
    p.row_tiles = ceil_div(N, FWD_RT);
    int slabs = ceil_div(SWEEP_TARGET_BLOCKS, p.row_tiles);
    if (slabs > p.chunks) slabs = p.chunks;
    if (slabs < 1) slabs = 1;
    p.chunks_per_slab = ceil_div(p.chunks, slabs);
    p.slabs = ceil_div(p.chunks, p.chunks_per_slab);
    return p;
}

// the kernels' batch template: 8 rows of LDS and registers for B <= 8, else all 32
inline int batch_nb(int B) { return B <= 8 ? 8 : TRAIN_MAX_B; }

// float4 loads and stores: every row starts 16-byte aligned (a null pointer is one the launch does not use)
inline bool vec_ok(int K, std::initializer_list<const void*> ptrs) {
    bool ok = K % 4 == 0;
    for (const void* p : ptrs) ok = ok && ((uintptr_t)p & 15u) == 0;
    return ok;
}

// the workspaces of dims = (I, H6, H7, O): the sweeps' dX partials [row tile][B][K] of fc7 and fc8, the forward's slab sums
// [slab][B][N] of every layer, and fc6's dX partials at a batch of B (vpk_train_step_dx)
inline size_t partial_bytes(const int dims[4]) {
    const size_t p7 = (size_t)plan_sweep(dims[2], dims[1]).tiles * TRAIN_MAX_B * dims[1];
    const size_t p8 = (size_t)plan_sweep(dims[3], dims[2]).tiles * TRAIN_MAX_B * dims[2];
    return (p7 > p8 ? p7 : p8) * 4;
}
inline size_t fpartial_bytes(const int dims[4]) {
    size_t fp = 0;
    for (int l = 0; l < 3; ++l) {
        const size_t want = (size_t)plan_fwd(dims[l + 1], dims[l]).slabs * TRAIN_MAX_B * dims[l + 1];
        if (want > fp) fp = want;
    }
    return fp * 4;
}
inline size_t xpartial_bytes(const int dims[4], int B) { return (size_t)plan_sweep(dims[1], dims[0]).tiles * B * dims[0] * 4; }

// ---- the conv stack -----------------------------------------------------------------------------------------------------
constexpr int CT_MAX_B = 32;
constexpr int CT_MAX_LAYERS = 32;
constexpr int CT_TILE = 64;           // a workgroup's tile of C: 64 x 64, one 32 x 32 quadrant per wave
constexpr int CT_CHUNK = 16;          // reduction terms staged in LDS at a time
constexpr int CT_LDS_ROW = CT_TILE + 4;
constexpr int CT_TARGET_BLOCKS = 1024;
constexpr int CT_LRN_PIX = 32;        // pixels of an LRN workgroup (x 8 channel lanes)
constexpr int CT_LRN_MAX_C = 512;     // 64 KiB of LDS

struct LayerShape {
    vpk_stack_layer d = {};
    int C = 0, H = 0, W = 0;          // input
    int OC = 0, OH = 0, OW = 0;       // output
    size_t out_size() const { return (size_t)OC * OH * OW; }
    size_t in_size() const { return (size_t)C * H * W; }
    size_t weights() const { return (size_t)OC * (C / d.groups) * d.kernel * d.kernel; }
};

// STACK_NO_CHAIN: a size, a divisibility or the layer count is off, or a blob's pixels of CT_MAX_B images do not index in
// int.  STACK_LRN_WIDE: the layers chain, but an LRN's channel column does not fit the kernel's LDS.
enum StackRule { STACK_OK = 0, STACK_NO_CHAIN, STACK_LRN_WIDE };

// the shapes of a chain, appended to `out` up to the first layer that does not chain
inline StackRule chain(int C, int H, int W, const vpk_stack_layer* layers, int n, std::vector<LayerShape>& out) {
    namespace ct = vpk_convtrain;
    bool wide = false;
    if (C < 1 || H < 1 || W < 1 || !layers || n < 1 || n > CT_MAX_LAYERS) return STACK_NO_CHAIN;
    for (int l = 0; l < n; ++l) {
        LayerShape L;
        L.d = layers[l];
        L.C = C; L.H = H; L.W = W;
        const vpk_stack_layer& d = L.d;
        if (d.kind == VPK_LAYER_CONV) {
            if (d.out_channels < 1 || d.kernel < 1 || d.stride < 1 || d.pad < 0 || d.groups < 1) return STACK_NO_CHAIN;
            if (C % d.groups || d.out_channels % d.groups) return STACK_NO_CHAIN;
            L.OC = d.out_channels;
            L.OH = ct::conv_out_size(H, d.kernel, d.stride, d.pad);
            L.OW = ct::conv_out_size(W, d.kernel, d.stride, d.pad);
        } else if (d.kind == VPK_LAYER_LRN) {
            if (d.local_size < 1 || d.local_size % 2 == 0) return STACK_NO_CHAIN;
            if (C > CT_LRN_MAX_C) wide = true;
            L.OC = C; L.OH = H; L.OW = W;
        } else if (d.kind == VPK_LAYER_POOL) {
            if (d.kernel < 1 || d.stride < 1) return STACK_NO_CHAIN;
            L.OC = C;
            L.OH = ct::pool_out_size(H, d.kernel, d.stride);
            L.OW = ct::pool_out_size(W, d.kernel, d.stride);
        } else {
            return STACK_NO_CHAIN;
        }
        if (L.OH < 1 || L.OW < 1) return STACK_NO_CHAIN;
        if ((double)L.OC * L.OH * L.OW * CT_MAX_B >= 2147483648.0) return STACK_NO_CHAIN;      // the kernels index pixels in int
        out.push_back(L);
        C = L.OC; H = L.OH; W = L.OW;
    }
    return wide ? STACK_LRN_WIDE : STACK_OK;
}

inline vpk_convtrain::ConvGeom geom(const LayerShape& L, int B) {
    vpk_convtrain::ConvGeom q;
    q.C = L.C; q.H = L.H; q.W = L.W;
    q.OC = L.OC; q.K = L.d.kernel; q.stride = L.d.stride; q.pad = L.d.pad; q.groups = L.d.groups; q.relu = L.d.relu ? 1 : 0;
    q.OH = L.OH; q.OW = L.OW; q.B = B;
    return q;
}

// grids: the products' (tiles of n, tiles of m, groups x slabs), the LRN's (pixel tiles, B) with its LDS column, and the
// 256-thread blocks of one thread per element (the pools, the update)
struct Grid { unsigned x, y, z; };
inline Grid gemm_grid(int mode, const vpk_convtrain::ConvGeom& q, int slabs) {
    int M, N, R;
    vpk_convtrain::gemm_dims(mode, q, M, N, R);
    return Grid{(unsigned)ceil_div(N, CT_TILE), (unsigned)ceil_div(M, CT_TILE), (unsigned)(q.groups * slabs)};
}
inline Grid lrn_grid(const LayerShape& L, int B) { return Grid{(unsigned)ceil_div(L.H * L.W, CT_LRN_PIX), (unsigned)B, 1u}; }
inline size_t lrn_lds_bytes(const LayerShape& L) { return (size_t)L.C * CT_LRN_PIX * 4; }
inline unsigned blocks_of(size_t elements) { return (unsigned)((elements + 255) / 256); }

// the weight gradient of a CONV layer at a batch: its slabs (convtrain_device.hpp's wgrad_slabs at the kernel's tile), the
// columns of a row of its partials (the taps and the bias) and the bytes of all slabs
struct WgradPlan { int slabs, slab_len, cols; size_t bytes; };
inline WgradPlan plan_wgrad(const LayerShape& L, int B) {
    const vpk_convtrain::ConvGeom q = geom(L, B);
    WgradPlan p;
    vpk_convtrain::wgrad_slabs(q, CT_TILE, CT_CHUNK, CT_TARGET_BLOCKS, p.slabs, p.slab_len);
    p.cols = q.ICg() * q.K * q.K + 1;
    p.bytes = (size_t)p.slabs * L.OC * p.cols * 4;
    return p;
}
// ... and the one buffer the layers (LayerShape or the driver's own type on top of it) of a batch share
template <class Layers>
size_t slab_buffer_bytes(const Layers& layers, int B) {
    size_t want = 0;
    for (const LayerShape& L : layers)
        if (L.d.kind == VPK_LAYER_CONV && plan_wgrad(L, B).bytes > want) want = plan_wgrad(L, B).bytes;
    return want;
}

// the kept blobs of B images: a layer's output (and gradient, scale, index: all 4-byte elements)
inline size_t blob_bytes(const LayerShape& L, int B) { return (size_t)B * L.out_size() * 4; }

// The life cycle of the kept blobs.  A forward clears them when it starts to launch and owns them once it is done; a
// backward needs a forward that no backward has consumed and consumes it; the outputs stay readable until the next forward,
// the gradients from a backward until the next forward.
struct KeptBlobs {
    int fwd_B = 0;                    // batch of the last forward that no backward has consumed (0: none)
    int blob_B = 0;                   // batch the kept blobs hold
    bool grads = false;               // the gradient blobs belong to the kept forward
    void forward_begins() { fwd_B = blob_B = 0; grads = false; }
    void forward_done(int B) { fwd_B = blob_B = B; }
    bool backward_allowed() const { return fwd_B >= 1; }
    void backward_done() { fwd_B = 0; grads = true; }
    bool read_allowed() const { return blob_B >= 1; }
    bool gradient_read_allowed() const { return grads; }
};

// ---- the solver ---------------------------------------------------------------------------------------------------------
// the float32 numbers the update kernels of an iteration get: the one caller of train_device.hpp's learning_rate
struct Rates { float lr_w, dec_w, lr_b, dec_b, mu; };
inline Rates rates(const vpk_train_params& p, long long iteration) {
    const float lr = vpk_train::learning_rate(p.base_lr, p.gamma, p.stepsize, iteration);
    return Rates{lr * p.lr_mult_weight, p.weight_decay * p.decay_mult_weight, lr * p.lr_mult_bias,
                 p.weight_decay * p.decay_mult_bias, p.momentum};
}

// vpk_convtrain_set_params ignores the dropout ratio; vpk_train_set_params divides by 1 - dropout_ratio
inline bool stack_params_ok(const vpk_train_params& p) { return p.stepsize >= 1; }
inline bool head_params_ok(const vpk_train_params& p) {
    return p.dropout_ratio >= 0.0f && p.dropout_ratio < 1.0f && stack_params_ok(p);
}

}  // namespace vpk_train_plan
#pragma GCC visibility pop

#endif
