// train_plan_driver.cpp -- TEST-ONLY stand-alone program over csrc/train_plan.hpp: the tables of tests/test_train_plan.py --
// the head's plans at the net's sizes and over a grid of sizes, the workspaces against every launch of a step, the stack's
// refusals and limits, its buffers, the kept blobs' life cycle, the rates and the set_params rules -- walked in one process.
// Made to be built with the host sanitizers and run on its own; it prints one line and returns 0 when every call answered as
// expected:
//     python tests/hostsim/hostbuild.py drivers
// No test runs it.
#include <stdio.h>

#include <vector>

#include "../../vanishing_points_2017_amd/csrc/train_plan.hpp"

using namespace vpk_train_plan;

namespace {

int failures = 0, calls = 0;

void expect(bool ok, const char* what) {
    ++calls;
    if (!ok) {
        ++failures;
        printf("FAILED: %s\n", what);
    }
}

vpk_stack_layer conv(int oc, int k, int stride = 1, int pad = 0, int groups = 1) {
    vpk_stack_layer d = {};
    d.kind = VPK_LAYER_CONV; d.out_channels = oc; d.kernel = k; d.stride = stride; d.pad = pad; d.groups = groups; d.relu = 1;
    return d;
}
vpk_stack_layer lrn(int n = 5) {
    vpk_stack_layer d = {};
    d.kind = VPK_LAYER_LRN; d.local_size = n; d.alpha = 1e-4f; d.beta = 0.75f; d.k = 1.0f;
    return d;
}
vpk_stack_layer pool(int k = 3, int stride = 2) {
    vpk_stack_layer d = {};
    d.kind = VPK_LAYER_POOL; d.kernel = k; d.stride = stride;
    return d;
}

StackRule rule_of(int C, int H, int W, const std::vector<vpk_stack_layer>& layers, std::vector<LayerShape>* out = nullptr) {
    std::vector<LayerShape> L;
    const StackRule r = chain(C, H, W, layers.data(), (int)layers.size(), L);
    if (out) *out = L;
    return r;
}

vpk_train_params defaults() {                     // vpk_train_default_params
    vpk_train_params p = {};
    p.base_lr = 1e-4f; p.gamma = 0.1f; p.stepsize = 200000; p.momentum = 0.9f; p.weight_decay = 5e-4f; p.lr_mult_weight = 1.0f;
    p.decay_mult_weight = 1.0f; p.lr_mult_bias = 2.0f; p.decay_mult_bias = 0.0f; p.dropout_ratio = 0.5f;
    return p;
}

void head_all() {
    const int net[3][7] = {{4096, 57600, 128, 32, 8, 29, 256}, {4096, 4096, 32, 128, 8, 2, 256}, {400, 4096, 16, 25, 16, 1, 25}};
    for (const auto& w : net) {
        const SweepPlan s = plan_sweep(w[0], w[1]);
        const FwdPlan f = plan_fwd(w[0], w[1]);
        expect(s.rt == w[2] && s.tiles == w[3] && f.slabs == w[4] && f.chunks_per_slab == w[5] && f.row_tiles == w[6], "the net's plans");
    }
    for (int n : {1, 7, 16, 17, 400})
        for (int k : {1, 4, 255, 256, 257, 4096}) {
            const SweepPlan s = plan_sweep(n, k);
            expect(s.rt % 8 == 0 && s.rt >= 16 && s.rt <= 128 && (s.tiles - 1) * s.rt < n && n <= s.tiles * s.rt, "sweep tiles");
            const FwdPlan f = plan_fwd(n, k);
            std::vector<int> seen((size_t)f.chunks, 0);
            for (int slab = 0; slab < f.slabs; ++slab) {
                expect(slab * f.chunks_per_slab < f.chunks, "no slab is empty");
                for (int c = slab * f.chunks_per_slab; c < f.chunks && c < (slab + 1) * f.chunks_per_slab; ++c) seen[(size_t)c] += 1;
            }
            bool once = true;
            for (int v : seen) once = once && v == 1;
            expect(once, "every chunk exactly once");
            const int variants[3][4] = {{k, n, 3, 5}, {2, k, n, 5}, {2, 3, k, n}};
            for (const auto& dims : variants)
                for (int B : {1, 8, 9, 32}) {
                    bool fits = true;
                    for (int l = 0; l < 3; ++l) {
                        const size_t N = (size_t)dims[l + 1], K = (size_t)dims[l];
                        fits = fits && (size_t)plan_fwd((int)N, (int)K).slabs * B * N * 4 <= fpartial_bytes(dims);
                        if (l > 0) fits = fits && (size_t)plan_sweep((int)N, (int)K).tiles * B * K * 4 <= partial_bytes(dims);
                    }
                    expect(fits && xpartial_bytes(dims, B) == (size_t)plan_sweep(dims[1], dims[0]).tiles * B * dims[0] * 4, "workspaces");
                }
            const char* base = (const char*)0x7f0000001000;
            for (int low : {0, 4, 8, 16})
                expect(vec_ok(k, {base, base + low, nullptr}) == (k % 4 == 0 && low % 16 == 0), "the float4 rule");
        }
    for (int B = 1; B <= 32; ++B) expect(batch_nb(B) == (B <= 8 ? 8 : 32), "the batch template");
}

void stack_all() {
    const std::vector<vpk_stack_layer> edge = {conv(8, 5, 2), lrn(), pool(), conv(12, 5, 1, 2, 2), lrn(), pool(), conv(16, 3, 1, 1),
                                               conv(16, 3, 1, 1, 2), conv(12, 3, 1, 1, 2), pool()};
    const int edge_shapes[10][3] = {{8, 22, 18}, {8, 22, 18}, {8, 11, 9}, {12, 11, 9}, {12, 11, 9}, {12, 5, 4}, {16, 5, 4}, {16, 5, 4},
                                    {12, 5, 4}, {12, 2, 2}};
    std::vector<LayerShape> L;
    expect(rule_of(1, 47, 39, edge, &L) == STACK_OK && L.size() == 10, "the edge stack chains");
    for (size_t l = 0; l < L.size(); ++l)
        expect(L[l].OC == edge_shapes[l][0] && L[l].OH == edge_shapes[l][1] && L[l].OW == edge_shapes[l][2], "the edge stack's shapes");
    for (int B : {1, 5, 32}) {
        size_t want = 0;
        for (const LayerShape& s : L) {
            if (s.d.kind != VPK_LAYER_CONV) continue;
            const WgradPlan w = plan_wgrad(s, B);
            expect(w.cols == s.C / s.d.groups * s.d.kernel * s.d.kernel + 1 && w.slabs >= 1 &&
                       (long long)w.slabs * w.slab_len >= (long long)B * s.OH * s.OW && w.bytes == (size_t)w.slabs * s.OC * w.cols * 4,
                   "a weight gradient's slabs");
            if (w.bytes > want) want = w.bytes;
            const Grid g = gemm_grid(vpk_convtrain::GEMM_WGRAD, geom(s, B), w.slabs);
            expect(g.x * 64u >= (unsigned)w.cols && g.y * 64u >= (unsigned)(s.OC / s.d.groups) && g.z == (unsigned)(s.d.groups * w.slabs),
                   "its grid");
        }
        expect(slab_buffer_bytes(L, B) == want && want > 0, "the slab buffer");
        expect(blob_bytes(L[9], B) == (size_t)B * 48 * 4 && lrn_grid(L[1], B).x == 13 && lrn_lds_bytes(L[1]) == 8 * 32 * 4, "blobs, LRN");
    }
    expect(rule_of(1, 2, 6, {pool(3)}) == STACK_NO_CHAIN, "a pool larger than its plane");
    expect(rule_of(1, 2, 6, {conv(4, 7)}) == STACK_NO_CHAIN, "a kernel larger than its plane");
    expect(rule_of(2, 6, 5, {conv(4, 3, 1, 0, 3)}) == STACK_NO_CHAIN, "groups that do not divide the input");
    expect(rule_of(2, 6, 5, {conv(6, 3, 1, 0, 4)}) == STACK_NO_CHAIN, "groups that do not divide the output");
    expect(rule_of(1, 2, 6, {lrn(4)}) == STACK_NO_CHAIN, "an even local_size");
    expect(rule_of(1, 2, 6, {conv(4, 3, 0)}) == STACK_NO_CHAIN, "stride 0");
    expect(rule_of(1, 2, 6, {conv(4, 3, 1, 1), pool(), pool(), pool(3)}) == STACK_NO_CHAIN, "pools past the plane");
    expect(rule_of(2, 6, 5, {}) == STACK_NO_CHAIN, "no layer");
    std::vector<LayerShape> none;
    expect(chain(2, 6, 5, nullptr, 1, none) == STACK_NO_CHAIN, "null layers");
    expect(rule_of(513, 2, 2, {lrn()}) == STACK_LRN_WIDE && rule_of(512, 2, 2, {lrn()}) == STACK_OK, "the LRN's LDS column");
    expect(rule_of(513, 2, 2, {lrn(), pool(3)}) == STACK_NO_CHAIN, "a chain that breaks is that first");
    expect(rule_of(1, 2, 2, std::vector<vpk_stack_layer>(32, lrn())) == STACK_OK, "32 layers");
    expect(rule_of(1, 2, 2, std::vector<vpk_stack_layer>(33, lrn())) == STACK_NO_CHAIN, "33 layers");
    expect(rule_of(1, 2731, 8191, {conv(3, 1)}) == STACK_OK, "2^26 - 1 elements per image");
    expect(rule_of(1, 8192, 8192, {conv(1, 1)}) == STACK_NO_CHAIN, "2^26 elements per image");
}

void kept_all() {
    KeptBlobs k;
    expect(!k.read_allowed() && !k.gradient_read_allowed() && !k.backward_allowed(), "nothing before a forward");
    k.forward_begins();
    k.forward_done(5);
    expect(k.read_allowed() && !k.gradient_read_allowed() && k.backward_allowed() && k.fwd_B == 5 && k.blob_B == 5, "a forward");
    k.backward_done();
    expect(k.read_allowed() && k.gradient_read_allowed() && !k.backward_allowed() && k.blob_B == 5, "a backward consumes it");
    k.forward_begins();
    expect(!k.read_allowed() && !k.gradient_read_allowed() && !k.backward_allowed(), "a forward refused after it began");
    k.forward_done(2);
    expect(k.read_allowed() && !k.gradient_read_allowed() && k.backward_allowed() && k.fwd_B == 2, "the next forward");
}

void solver_all() {
    vpk_train_params p = defaults();
    const long long its[5] = {0, 2, 3, 6, 200000};
    for (int set = 0; set < 2; ++set) {
        for (long long it : its) {
            float lr = p.base_lr;
            for (long long n = it / p.stepsize; n > 0 && lr != 0.0f; --n) lr *= p.gamma;
            const Rates r = rates(p, it);
            expect(r.lr_w == lr * p.lr_mult_weight && r.lr_b == lr * p.lr_mult_bias && r.dec_w == p.weight_decay * p.decay_mult_weight &&
                       r.dec_b == p.weight_decay * p.decay_mult_bias && r.mu == p.momentum, "rates");
        }
        p.gamma = 0.5f;
        p.stepsize = 3;
    }
    const float ratios[4] = {-0.1f, 0.0f, 0.999f, 1.0f};
    const bool head[4] = {false, true, true, false};
    for (int k = 0; k < 4; ++k) {
        vpk_train_params q = defaults();
        q.dropout_ratio = ratios[k];
        expect(head_params_ok(q) == head[k] && stack_params_ok(q), "dropout_ratio");
    }
    vpk_train_params q = defaults();
    q.stepsize = 0;
    expect(!head_params_ok(q) && !stack_params_ok(q), "stepsize 0");
    q.stepsize = 1;
    expect(head_params_ok(q) && stack_params_ok(q), "stepsize 1");
}

}  // namespace

int main() {
    head_all();
    stack_all();
    kept_all();
    solver_all();
    printf("train_plan_driver: %d checks, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
