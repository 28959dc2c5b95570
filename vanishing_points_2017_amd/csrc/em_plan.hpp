// em_plan.hpp -- what vpk_em_batch (vpk_em.hip) decides on the host before it launches anything: the rules a call is held
// to, the slot and workgroup count, the time-sliced session's geometry and its refusals, the layout of the session buffer and
// of the device header, and the order the images are queued in.  Pure functions of the call's arguments and of a few facts
// of the handle (EmFacts); no HIP call and no HIP include of its own: tests/hostsim/sim_em_plan.cpp compiles it for the CPU
// tests (tests/test_em_plan.py) with hip_sim.hpp in front, as sim_em.cpp compiles em_ctx.hpp.
#ifndef VPK_EM_PLAN_HPP_
#define VPK_EM_PLAN_HPP_

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>

#include "em_ctx.hpp"

namespace vpk {

constexpr int EM_THREADS = 512;   // 8 waves: 2 per SIMD
constexpr int EM_WAVES = EM_THREADS / 64;
// when a batch leaves at most one workgroup per CU, the workgroup takes (almost) the whole 160 KiB so
// that the smoother's operand panel of any YUD/ECD-sized image fits and lsim is read once per E-step
constexpr int WT_DOUBLES_BIG = (int)((163840 - SH_BYTES) / sizeof(double)) / 32 * 32;   // everything a CU has (~147 KiB)
constexpr size_t EM_LDS_BYTES_BIG = SH_BYTES + WT_DOUBLES_BIG * sizeof(double);
static_assert(EM_LDS_BYTES_BIG <= 163840, "LDS per CU");
constexpr long long EM_MAX_LINES = 46000;   // per image
constexpr size_t EM_SESS_HEAD = 256;        // the session's counters

// One workgroup per CU (vpk_em.hip: EM_BOUND), with the whole remaining LDS (128 KiB) as the smoother's operand
// panel: single-pass smoothing for every image whose N x W panel fits.
struct EmMode { int per_cu; int wt_doubles; size_t lds_bytes; };
inline EmMode em_mode(int lds_doubles) {
    if (lds_doubles <= 0) return EmMode{1, WT_DOUBLES_BIG, EM_LDS_BYTES_BIG};
    // vpk_em_set_lds_panel: the budget the phases PLAN with; the launch still gets at least the setup phases' scratch
    const int wt = std::min(std::max(lds_doubles, 64), WT_DOUBLES_BIG);
    return EmMode{1, wt, SH_BYTES + (size_t)std::max(wt, PART_DOUBLES) * sizeof(double)};
}

// what the plan reads of the handle
struct EmFacts {
    int cu_share, max_workgroups;   // vpk_em_set_workgroups (0 = no cap)
    size_t total_mem;
    int lds_doubles;                // vpk_em_set_lds_panel
    double slice_ms; int slice_nmax;   // vpk_em_set_time_slice (0 = off)
    int started_cap, wait_cap;      // capacities of the parked-image lists
    // a live session, and the geometry its parked images were laid out with
    bool has_sess; size_t sess_slot_bytes; int sess_slots, sess_wgs; EmLayout sess_layout;
    bool unflushed;                 // parked images may exist
    size_t ws_bytes;                // the workspace the handle holds
};

enum EmRule {                       // in the order the driver checks them
    EM_PLAN_OK = 0,
    EM_PLAN_NULL,                   // null buffer or batch < 1
    EM_PLAN_SPHERE,                 // sphere_size or max_vp
    EM_PLAN_PARAMS, EM_PLAN_NUM_ITER, EM_PLAN_FREQ, EM_PLAN_NUM_INIT, EM_PLAN_N_INIT,   // params null, or one of its rules
    EM_PLAN_OFFSETS,                // not monotone
    EM_PLAN_LINES,                  // an image beyond EM_MAX_LINES
    EM_PLAN_SLICE_MEM,              // the sliced session's slots beyond half of the memory
    EM_PLAN_SESS_CHANGED,           // the slot layout changed while images are parked
    EM_PLAN_WS_MOVES,               // the workspace would move while images are parked
};

inline int em_rule_code(EmRule r) {
    return r == EM_PLAN_OK ? VPK_OK : r >= EM_PLAN_SESS_CHANGED ? VPK_ERR_STATE
         : r == EM_PLAN_NUM_INIT || r == EM_PLAN_N_INIT || r == EM_PLAN_LINES || r == EM_PLAN_SLICE_MEM ? VPK_ERR_LIMIT : VPK_ERR_ARG;
}

struct EmPlan {
    EmRule rule = EM_PLAN_OK;
    EmMode mode = {};
    bool sliced = false;
    int mcap = 0, slots = 0, wgs = 0;
    EmLayout L = {};                // (a refused plan holds zeros here)
    size_t slot_bytes = 0;
    bool new_session = false;       // sliced: no session yet, or its geometry differs from this call's
    size_t off_bytes = 0, ord_bytes = 0;   // device header: offsets (B+1 i64) | order (B i32) | queue counter (256 bytes)
    size_t ws_bytes() const { return (size_t)slots * slot_bytes; }
    size_t staged_bytes() const { return off_bytes + ord_bytes; }   // what is uploaded; the counter behind it is zeroed on the device
};

// Slots and workgroups for `batch` images of at most nmax lines.  Unsliced, every workgroup owns one slot: no more than
// images, halved while they claim more than half of HBM.  The workgroups of a sliced launch also resume what earlier launches
// parked, so their number does not follow the batch, and slots outlive the launch: running (<= wgs) + parked and not yet
// resumed (<= wgs), see EmSliceArgs.  An unsliced call flushes first, so only a sliced one meets parked images.
inline EmPlan em_plan_slots(const EmFacts& f, int batch, long long nmax, const vpk_em_params& p, int n_init, bool has_init,
                            bool sliced) {
    EmPlan pl;
    pl.mode = em_mode(f.lds_doubles);
    pl.sliced = sliced;
    if (sliced && (long long)f.slice_nmax > nmax) nmax = f.slice_nmax;
    pl.mcap = em_mcap(p.num_init_vp, n_init, has_init, p.do_split != 0, p.num_iter, p.split_merge_freq, MAXM);
    pl.L = em_layout((int)nmax, pl.mcap, EM_WAVES, p.use_weights != 0, p.do_split != 0);
    pl.slot_bytes = pl.L.total_doubles * sizeof(double);
    pl.wgs = f.cu_share * pl.mode.per_cu;                // one workgroup per CU of the handle's share, under the cap
    if (f.max_workgroups > 0 && pl.wgs > f.max_workgroups) pl.wgs = f.max_workgroups;
    const size_t budget = f.total_mem / 2;               // never claim more than half of HBM
    if (!sliced) {
        int slots = std::min(pl.wgs, batch);
        while (slots > 1 && (size_t)slots * pl.slot_bytes > budget) slots /= 2;
        pl.slots = pl.wgs = slots < 1 ? 1 : slots;
        return pl;
    }
    pl.slots = 2 * pl.wgs + 8;
    pl.new_session = !(f.has_sess && f.sess_slot_bytes == pl.slot_bytes && f.sess_slots == pl.slots && f.sess_wgs == pl.wgs &&
                       memcmp(&f.sess_layout, &pl.L, sizeof(pl.L)) == 0);
    if (pl.ws_bytes() > budget) pl.rule = EM_PLAN_SLICE_MEM;
    else if (pl.new_session && f.unflushed) pl.rule = EM_PLAN_SESS_CHANGED;
    else if (f.unflushed && pl.ws_bytes() > f.ws_bytes) pl.rule = EM_PLAN_WS_MOVES;
    return pl;
}

// The plan of one vpk_em_batch call.  buffers: every required pointer but offsets and params is given; has_init: init_vp is.
inline EmPlan em_plan(const EmFacts& f, int batch, const int64_t* offsets, bool buffers, int sphere_size, int max_vp,
                      const vpk_em_params* p, int n_init, bool has_init) {
    EmPlan bad;
    auto fail = [&bad](EmRule r) { bad.rule = r; return bad; };
    if (batch < 1 || !offsets || !buffers) return fail(EM_PLAN_NULL);
    if (sphere_size < GRIDN || max_vp < 1) return fail(EM_PLAN_SPHERE);
    if (!p) return fail(EM_PLAN_PARAMS);
    if (p->num_iter < 1 || p->num_iter > 100000) return fail(EM_PLAN_NUM_ITER);
    if (p->split_merge_freq < 1) return fail(EM_PLAN_FREQ);
    if (p->num_init_vp < 1 || p->num_init_vp > MAXM) return fail(EM_PLAN_NUM_INIT);
    if (has_init && (n_init < 1 || n_init > MAXM)) return fail(EM_PLAN_N_INIT);
    long long nmax = 0;
    for (int b = 0; b < batch; ++b) {
        const long long n = offsets[b + 1] - offsets[b];
        if (n < 0) return fail(EM_PLAN_OFFSETS);
        nmax = std::max(nmax, n);
    }
    if (nmax > EM_MAX_LINES) return fail(EM_PLAN_LINES);
    EmPlan pl = em_plan_slots(f, batch, nmax, *p, n_init, has_init, f.slice_ms > 0.0);
    pl.off_bytes = em_align((size_t)(batch + 1) * 8, 256);
    pl.ord_bytes = em_align((size_t)batch * 4, 256);
    return pl;
}

// the queue order: largest image first, ties in index order
inline void em_order(int batch, const int64_t* offsets, int* order) {
    std::iota(order, order + batch, 0);
    std::stable_sort(order, order + batch, [&](int x, int y) { return offsets[x + 1] - offsets[x] > offsets[y + 1] - offsets[y]; });
}

// session buffer: [counters | slot flags | started list A, B | waiting list A, B], byte offsets, every region 256-aligned;
// carry_bytes: sizeof of a list entry (EmCarry, vpk_em.hip)
struct EmSessLayout { size_t head, busy, started[2], waiting[2], total; };
inline EmSessLayout em_sess_layout(int slots, int started_cap, int wait_cap, size_t carry_bytes) {
    const size_t sb = em_align(carry_bytes * started_cap, 256), wb = em_align(carry_bytes * wait_cap, 256);
    const size_t lists = EM_SESS_HEAD + em_align((size_t)slots * 4, 256);
    return EmSessLayout{0, EM_SESS_HEAD, {lists, lists + sb}, {lists + 2 * sb, lists + 2 * sb + wb}, lists + 2 * sb + 2 * wb};
}

// a launch's slice in clock ticks (0 = no deadline), at least 1 for a positive slice
inline long long em_slice_ticks(double slice_ms) {
    const long long t = slice_ms > 0 ? (long long)(slice_ms * 1e-3 / (CLOCK_US * 1e-6)) : 0;
    return slice_ms > 0 && t < 1 ? 1 : t;
}

}  // namespace vpk
#endif
