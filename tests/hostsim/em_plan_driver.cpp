// em_plan_driver.cpp -- TEST-ONLY stand-alone program over csrc/em_plan.hpp: the cases of tests/test_em_plan.py -- slots with
// and without a time slice, the session's refusals, every limit, the header and session layouts, the queue order -- walked in
// one process.  Made to be built with the host sanitizers and run on its own; it prints one line and returns 0 when every
// call answered as expected:
//     python tests/hostsim/hostbuild.py drivers
// No test runs it.
#include <stdio.h>

#include <vector>

#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/em_plan.hpp"

using namespace vpk;

namespace {

int failures = 0, calls = 0;

void expect(bool ok, const char* what) {
    ++calls;
    if (!ok) {
        ++failures;
        printf("FAILED: %s\n", what);
    }
}

vpk_em_params defaults() {                        // vpk_em_default_params
    vpk_em_params p = {};
    p.num_iter = 100; p.do_merge = 1; p.do_split = 1; p.do_iterations = 1; p.use_weights = 1; p.num_init_vp = 25;
    p.split_merge_freq = 10; p.num_min_lines = 3; p.wbias = 1.0; p.merge_thresh = 1e-3; p.outlier_thresh = 1.96 * 1.96;
    p.final_convergence = 5e-3; p.s_thresh = 1e-200;
    return p;
}

EmFacts facts(int cap = 0, double slice_ms = 0.0, int slice_nmax = 0, size_t total_mem = (size_t)288 << 30) {
    EmFacts f = {};
    f.cu_share = 256; f.max_workgroups = cap; f.total_mem = total_mem; f.slice_ms = slice_ms; f.slice_nmax = slice_nmax;
    f.started_cap = 1024; f.wait_cap = 8192;
    return f;
}

struct Call {
    std::vector<int64_t> off;
    vpk_em_params p = defaults();
    bool buffers = true, null_params = false, has_init = false;
    int sphere_size = 500, max_vp = 64, n_init = 0;
    explicit Call(const std::vector<int64_t>& sizes) : off(sizes.size() + 1, 0) {
        for (size_t b = 0; b < sizes.size(); ++b) off[b + 1] = off[b] + sizes[b];
    }
    EmPlan plan(const EmFacts& f) const {
        return em_plan(f, (int)off.size() - 1, off.data(), buffers, sphere_size, max_vp, null_params ? nullptr : &p, n_init, has_init);
    }
};

EmFacts parked(const EmFacts& f, const EmPlan& pl) {
    EmFacts g = f;
    g.has_sess = true; g.sess_slot_bytes = pl.slot_bytes; g.sess_slots = pl.slots; g.sess_wgs = pl.wgs; g.sess_layout = pl.L;
    g.unflushed = true; g.ws_bytes = pl.ws_bytes();
    return g;
}

void slots_all() {
    const size_t s = Call({380}).plan(facts()).slot_bytes;
    const int want[5][3] = {{1, 0, 1}, {102, 0, 102}, {300, 0, 256}, {102, 30, 30}, {300, 1000, 256}};   // batch, cap, slots
    for (const auto& w : want) {
        const EmPlan pl = Call(std::vector<int64_t>((size_t)w[0], 380)).plan(facts(w[1]));
        expect(pl.rule == EM_PLAN_OK && pl.slots == w[2] && pl.wgs == w[2] && pl.ws_bytes() == (size_t)w[2] * s, "unsliced slots");
    }
    const Call yud(std::vector<int64_t>(102, 380));
    expect(yud.plan(facts(0, 0.0, 0, 4 * s)).slots == 1, "halved down to 1");
    expect(yud.plan(facts(0, 0.0, 0, 2 * 102 * s)).slots == 102, "exactly half of the memory");
    expect(yud.plan(facts(0, 0.0, 0, 2 * 102 * s - 2)).slots == 51, "one halving");
    const EmPlan one = yud.plan(facts(0, 0.0, 0, s));
    expect(one.rule == EM_PLAN_OK && one.slots == 1, "a slot beyond half of the memory");
    const vpk_em_params p = defaults();
    expect(em_plan_slots(facts(), 300, 380, p, 0, false, false).ws_bytes() == 256 * s, "vpk_em_workspace_bytes");
}

void sliced_all() {
    const size_t s = Call({12}).plan(facts()).slot_bytes;
    for (int cap : {0, 24}) {
        const int wgs = cap ? cap : 256;
        const EmPlan pl = Call({12, 12, 12}).plan(facts(cap, 5.0));
        expect(pl.rule == EM_PLAN_OK && pl.sliced && pl.new_session && pl.wgs == wgs && pl.slots == 2 * wgs + 8, "sliced slots");
    }
    expect(Call({12, 40}).plan(facts(0, 5.0, 100)).L.ldn == 104, "slice_nmax above the largest image");
    expect(Call({12, 40}).plan(facts(0, 5.0, 20)).L.ldn == 40, "slice_nmax below it");
    expect(Call({12}).plan(facts(0, 5.0, 0, 2 * 520 * s)).rule == EM_PLAN_OK, "sliced slots at half of the memory");
    expect(Call({12}).plan(facts(0, 5.0, 0, 2 * 520 * s - 2)).rule == EM_PLAN_SLICE_MEM, "sliced slots beyond it");
    const EmFacts f0 = facts(24, 5.0, 40);
    const Call call({12, 40});
    const EmPlan first = call.plan(f0);
    const EmFacts f = parked(f0, first);
    expect(call.plan(f).rule == EM_PLAN_OK && !call.plan(f).new_session, "the same geometry joins the session");
    for (int k = 0; k < 5; ++k) {
        EmFacts g = f;
        if (k == 0) g.has_sess = false;
        if (k == 1) g.sess_slot_bytes += 1;
        if (k == 2) g.sess_slots += 1;
        if (k == 3) g.sess_wgs += 1;
        if (k == 4) g.sess_layout.part += 8;
        expect(call.plan(g).rule == EM_PLAN_SESS_CHANGED, "a session fact changed while images are parked");
        g.unflushed = false;
        expect(call.plan(g).rule == EM_PLAN_OK && call.plan(g).new_session, "... and with nothing parked");
    }
    expect(Call({12, 41}).plan(f).rule == EM_PLAN_SESS_CHANGED, "more lines than the slots hold");
    EmFacts g = f;
    g.ws_bytes = first.ws_bytes() - 1;
    expect(call.plan(g).rule == EM_PLAN_WS_MOVES, "the workspace one byte short");
    g.slice_ms = 0.0;
    const EmPlan flushed = Call(std::vector<int64_t>(40, 41)).plan(g);
    expect(flushed.rule == EM_PLAN_OK && !flushed.sliced && flushed.slots == 24 && flushed.L.ldn == 48, "unsliced with parked images");
}

void limits_all() {
    const EmFacts f = facts();
    expect(Call({12, 46000}).plan(f).rule == EM_PLAN_OK, "46000 lines");
    expect(Call({12, 46001}).plan(f).rule == EM_PLAN_LINES, "46001 lines");
    Call dec({12, 12, 12});
    dec.off[3] = 20;
    expect(dec.plan(f).rule == EM_PLAN_OFFSETS, "offsets that decrease at the last image");
    const int iters[4] = {0, 100001, 1, 100000}, inits[4] = {0, 65, 1, 64};
    for (int k = 0; k < 4; ++k) {
        Call c({12});
        c.p.num_iter = iters[k];
        expect(c.plan(f).rule == (k < 2 ? EM_PLAN_NUM_ITER : EM_PLAN_OK), "num_iter");
        c.p = defaults();
        c.p.num_init_vp = inits[k];
        expect(c.plan(f).rule == (k < 2 ? EM_PLAN_NUM_INIT : EM_PLAN_OK), "num_init_vp");
        c.p = defaults();
        c.n_init = inits[k];
        expect(c.plan(f).rule == EM_PLAN_OK, "n_init without init_vp");
        c.has_init = true;
        expect(c.plan(f).rule == (k < 2 ? EM_PLAN_N_INIT : EM_PLAN_OK), "n_init with init_vp");
    }
    Call c({12});
    c.p.split_merge_freq = 0;
    expect(c.plan(f).rule == EM_PLAN_FREQ, "split_merge_freq 0");
    c.p.split_merge_freq = 1;
    expect(c.plan(f).rule == EM_PLAN_OK && c.plan(f).mcap == 64, "split_merge_freq 1");
    expect(Call({12}).plan(f).mcap == 40, "the default mcap");
    c.null_params = true;
    expect(c.plan(f).rule == EM_PLAN_PARAMS, "null params");
    c.max_vp = 0;
    expect(c.plan(f).rule == EM_PLAN_SPHERE, "max_vp 0");
    c.max_vp = 64; c.sphere_size = 19;
    expect(c.plan(f).rule == EM_PLAN_SPHERE, "sphere_size 19");
    c.buffers = false;
    expect(c.plan(f).rule == EM_PLAN_NULL, "a null buffer");
    expect(Call(std::vector<int64_t>()).plan(f).rule == EM_PLAN_NULL, "batch 0");
    expect(em_plan(f, 1, nullptr, true, 500, 64, &c.p, 0, false).rule == EM_PLAN_NULL, "null offsets");
    for (int r = EM_PLAN_OK; r <= EM_PLAN_WS_MOVES; ++r) {
        const int code = em_rule_code((EmRule)r);
        expect(r == EM_PLAN_OK ? code == VPK_OK : code == VPK_ERR_ARG || code == VPK_ERR_LIMIT || code == VPK_ERR_STATE, "codes");
    }
}

void layouts_all() {
    const int batches[4] = {31, 32, 64, 65};
    const size_t off[4] = {256, 512, 768, 768}, ord[4] = {256, 256, 256, 512};
    for (int k = 0; k < 4; ++k) {
        const EmPlan pl = Call(std::vector<int64_t>((size_t)batches[k], 12)).plan(facts());
        expect(pl.off_bytes == off[k] && pl.ord_bytes == ord[k] && pl.staged_bytes() == off[k] + ord[k], "header layout");
    }
    const Call ragged({5, 9, 5, 0, 9, 12, 0});
    std::vector<int> order(7, -7);
    em_order(7, ragged.off.data(), order.data());
    expect(order == std::vector<int>({5, 1, 4, 0, 2, 3, 6}), "largest first, ties in index order, empty images last");
    expect(ragged.plan(facts()).rule == EM_PLAN_OK, "images without lines");
    const int caps[2][2] = {{1024, 8192}, {3, 2}};
    for (const auto& c : caps)
        for (int slots : {1, 56, 65, 520}) {
            const size_t carry = 600;
            const EmSessLayout s = em_sess_layout(slots, c[0], c[1], carry);
            const size_t at[7] = {s.head, s.busy, s.started[0], s.started[1], s.waiting[0], s.waiting[1], s.total};
            const size_t size[6] = {24, (size_t)slots * 4, carry * c[0], carry * c[0], carry * c[1], carry * c[1]};
            for (int k = 0; k < 6; ++k)
                expect(at[k] % 256 == 0 && at[k] + size[k] <= at[k + 1] && at[k + 1] < at[k] + size[k] + 256, "session layout");
        }
    expect(em_slice_ticks(0.0) == 0 && em_slice_ticks(1e-9) == 1 && em_slice_ticks(2.5) >= 249999 && em_slice_ticks(2.5) <= 250001,
           "slice budget");
}

}  // namespace

int main() {
    slots_all();
    sliced_all();
    limits_all();
    layouts_all();
    printf("em_plan_driver: %d checks, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
