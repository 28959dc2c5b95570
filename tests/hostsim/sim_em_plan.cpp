// sim_em_plan.cpp -- TEST-ONLY host build of csrc/em_plan.hpp: what vpk_em_batch decides before it launches -- the rules,
// the slots and workgroups, the sliced session's refusals, the session and header layouts, the queue order -- callable from
// the CPU tests (tests/test_em_plan.py).  hip_sim.hpp stands in for the device vocabulary em_ctx.hpp is written against.
#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/em_plan.hpp"

using namespace vpk;

extern "C" {

struct SimEmPlan {
    int rule, code, sliced, mcap, slots, wgs, new_session, per_cu, wt_doubles;
    unsigned long long slot_bytes, ws_bytes, off_bytes, ord_bytes, staged_bytes, lds_bytes;
    EmLayout L;
};

// sizes of the structures tests/hostsim/simlib_em_plan.py mirrors
void sim_em_plan_sizes(int* out) {
    out[0] = (int)sizeof(EmFacts); out[1] = (int)sizeof(EmLayout); out[2] = (int)sizeof(SimEmPlan); out[3] = (int)sizeof(vpk_em_params);
}

static void fill(const EmPlan& pl, SimEmPlan* o) {
    *o = SimEmPlan{pl.rule, em_rule_code(pl.rule), pl.sliced, pl.mcap, pl.slots, pl.wgs, pl.new_session, pl.mode.per_cu,
                   pl.mode.wt_doubles, pl.slot_bytes, pl.ws_bytes(), pl.off_bytes, pl.ord_bytes, pl.staged_bytes(),
                   pl.mode.lds_bytes, pl.L};
}

// em_plan for one vpk_em_batch call; returns the rule
int sim_em_plan(const EmFacts* f, int batch, const int64_t* offsets, int buffers, int sphere_size, int max_vp,
                const vpk_em_params* p, int n_init, int has_init, SimEmPlan* out) {
    fill(em_plan(*f, batch, offsets, buffers != 0, sphere_size, max_vp, p, n_init, has_init != 0), out);
    return out->rule;
}

// what vpk_em_workspace_bytes computes
void sim_em_workspace(const EmFacts* f, int batch, int n_max, const vpk_em_params* p, int n_init, SimEmPlan* out) {
    fill(em_plan_slots(*f, batch, n_max, *p, n_init, n_init > 0, false), out);
}

void sim_em_order(int batch, const int64_t* offsets, int* order) { em_order(batch, offsets, order); }

// out: head, busy, started A, B, waiting A, B, total
void sim_em_sess_layout(int slots, int started_cap, int wait_cap, unsigned long long carry_bytes, unsigned long long* out) {
    const EmSessLayout s = em_sess_layout(slots, started_cap, wait_cap, (size_t)carry_bytes);
    const size_t v[7] = {s.head, s.busy, s.started[0], s.started[1], s.waiting[0], s.waiting[1], s.total};
    for (int k = 0; k < 7; ++k) out[k] = v[k];
}

long long sim_em_slice_ticks(double slice_ms) { return em_slice_ticks(slice_ms); }

}  // extern "C"
