// sim_train_plan.cpp -- TEST-ONLY host build of csrc/train_plan.hpp: what vpk_train.hip and vpk_convtrain.hip decide before
// they launch -- the head's plans and workspace sizes, the stack's shapes, limits, grids and buffers, the kept blobs' life
// cycle, the solver's rates and the set_params rules -- callable from the CPU tests (tests/test_train_plan.py).
#include "../../vanishing_points_2017_amd/csrc/train_plan.hpp"

using namespace vpk_train_plan;

extern "C" {

// sizes of the structures tests/hostsim/simlib_train_plan.py mirrors, and the constants it states
void sim_tp_constants(int* out) {
    const int v[12] = {(int)sizeof(vpk_train_params), (int)sizeof(vpk_stack_layer), TRAIN_MAX_B, FWD_RT, SWEEP_KT, SWEEP_MIN_RT,
                       SWEEP_MAX_RT, CT_MAX_B, CT_MAX_LAYERS, CT_TILE, CT_LRN_PIX, CT_LRN_MAX_C};
    for (int k = 0; k < 12; ++k) out[k] = v[k];
}

// out: rows per tile, tiles, column tiles
void sim_tp_sweep(int N, int K, int* out) {
    const SweepPlan p = plan_sweep(N, K);
    out[0] = p.rt; out[1] = p.tiles; out[2] = p.col_tiles;
}

// out: chunks, chunks per slab, slabs, row tiles
void sim_tp_fwd(int N, int K, int* out) {
    const FwdPlan p = plan_fwd(N, K);
    out[0] = p.chunks; out[1] = p.chunks_per_slab; out[2] = p.slabs; out[3] = p.row_tiles;
}

int sim_tp_nb(int B) { return batch_nb(B); }

// the pointers as integers: nothing is dereferenced
int sim_tp_vec(int K, unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d) {
    return vec_ok(K, {(const void*)(uintptr_t)a, (const void*)(uintptr_t)b, (const void*)(uintptr_t)c, (const void*)(uintptr_t)d});
}

// out: bytes of partial, fpartial and (at a batch of B) xpartial
void sim_tp_workspaces(const int* dims, int B, unsigned long long* out) {
    out[0] = partial_bytes(dims); out[1] = fpartial_bytes(dims); out[2] = xpartial_bytes(dims, B);
}

// the rule; shapes: (OC, OH, OW) of every layer that chained, *count of them
int sim_tp_chain(int C, int H, int W, const vpk_stack_layer* layers, int n, int* shapes, int* count) {
    std::vector<LayerShape> L;
    const StackRule rule = chain(C, H, W, layers, n, L);
    *count = (int)L.size();
    for (size_t l = 0; l < L.size(); ++l) {
        shapes[3 * l] = L[l].OC; shapes[3 * l + 1] = L[l].OH; shapes[3 * l + 2] = L[l].OW;
    }
    return (int)rule;
}

// Of layer `l` of a stack that chains, at a batch of B.  out: the slabs, their length, the columns and the bytes of a CONV
// layer's weight gradient; the three products' grids (FWD, DGRAD, WGRAD at those slabs: x, y, z each); the LRN's grid (x, y)
// and LDS bytes; the blob's bytes; the weights' count
void sim_tp_layer(int C, int H, int W, const vpk_stack_layer* layers, int n, int l, int B, unsigned long long* out) {
    std::vector<LayerShape> L;
    chain(C, H, W, layers, n, L);
    const LayerShape& s = L[(size_t)l];
    int k = 0;
    if (s.d.kind == VPK_LAYER_CONV) {
        const WgradPlan w = plan_wgrad(s, B);
        out[k++] = w.slabs; out[k++] = w.slab_len; out[k++] = w.cols; out[k++] = w.bytes;
        for (int mode = 0; mode < 3; ++mode) {
            const Grid g = gemm_grid(mode, geom(s, B), mode == vpk_convtrain::GEMM_WGRAD ? w.slabs : 1);
            out[k++] = g.x; out[k++] = g.y; out[k++] = g.z;
        }
    } else {
        k = 13;
    }
    const Grid g = lrn_grid(s, B);
    out[k++] = g.x; out[k++] = g.y; out[k++] = lrn_lds_bytes(s);
    out[k++] = blob_bytes(s, B);
    out[k++] = s.d.kind == VPK_LAYER_CONV ? s.weights() : 0;
}

unsigned long long sim_tp_slab_buffer(int C, int H, int W, const vpk_stack_layer* layers, int n, int B) {
    std::vector<LayerShape> L;
    chain(C, H, W, layers, n, L);
    return slab_buffer_bytes(L, B);
}

// The kept blobs through a list of events -- 0: a forward begins to launch, B > 0: it is done at a batch of B, -1: a backward
// is done -- then out: backward allowed, read allowed, gradient read allowed, the batch a backward would take, the batch a
// read would copy
void sim_tp_kept(const int* events, int n, int* out) {
    KeptBlobs k;
    for (int i = 0; i < n; ++i) {
        if (events[i] == 0) k.forward_begins();
        else if (events[i] > 0) k.forward_done(events[i]);
        else k.backward_done();
    }
    out[0] = k.backward_allowed(); out[1] = k.read_allowed(); out[2] = k.gradient_read_allowed(); out[3] = k.fwd_B; out[4] = k.blob_B;
}

// out: lr_w, dec_w, lr_b, dec_b, mu
void sim_tp_rates(const vpk_train_params* p, long long iteration, float* out) {
    const Rates r = rates(*p, iteration);
    out[0] = r.lr_w; out[1] = r.dec_w; out[2] = r.lr_b; out[3] = r.dec_b; out[4] = r.mu;
}

int sim_tp_params_ok(const vpk_train_params* p, int head) { return head ? head_params_ok(*p) : stack_params_ok(*p); }

}  // extern "C"
