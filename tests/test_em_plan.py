"""csrc/em_plan.hpp -- what vpk_em_batch (vpk_em.hip) decides on the host before it launches: the rules a call is held to,
the slots and workgroups, the time-sliced session's refusals, the session and header layouts and the queue order -- compiled
for the host by tests/hostsim/sim_em_plan.cpp, every rule at its edge.  The expectations are written out here from the rules,
not read back from the header.  CPU only: no GPU, no libvpk.so."""
import pytest

from hostsim import simlib_em_plan as sim

(OK, NULL, SPHERE, PARAMS, NUM_ITER, FREQ, NUM_INIT, N_INIT, OFFSETS, LINES, SLICE_MEM, SESS_CHANGED,
 WS_MOVES) = range(13)                                               # EmRule, in the order the driver checks them
VPK_OK, VPK_ERR_ARG, VPK_ERR_STATE, VPK_ERR_LIMIT = 0, -1, -4, -5    # include/vpk.h
CODE = {OK: VPK_OK, NULL: VPK_ERR_ARG, SPHERE: VPK_ERR_ARG, PARAMS: VPK_ERR_ARG, NUM_ITER: VPK_ERR_ARG, FREQ: VPK_ERR_ARG,
        NUM_INIT: VPK_ERR_LIMIT, N_INIT: VPK_ERR_LIMIT, OFFSETS: VPK_ERR_ARG, LINES: VPK_ERR_LIMIT, SLICE_MEM: VPK_ERR_LIMIT,
        SESS_CHANGED: VPK_ERR_STATE, WS_MOVES: VPK_ERR_STATE}
YUD = [380] * 102                                                    # a batch of the benchmark's shape


def align(x, a):
    return (x + a - 1) // a * a


def refused(p, rule):
    return (p.rule, p.code) == (rule, CODE[rule])


def slot_bytes(n):
    """bytes of a slot for images of n lines under the default parameters: em_layout.hpp's, passed through by the plan"""
    p = sim.plan(sim.facts(), [n])
    assert p.rule == OK and p.slot_bytes == p.L.total_doubles * 8 and p.slot_bytes % 256 == 0 and p.L.ldn == align(n, 8)
    return p.slot_bytes


# ---- slots, unsliced --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch, cap, slots", [(1, 0, 1), (102, 0, 102), (300, 0, 256), (102, 30, 30), (300, 1000, 256)])
def test_slots_are_the_least_of_cus_cap_and_batch(batch, cap, slots):
    p = sim.plan(sim.facts(cu_share=256, cap=cap), [380] * batch)
    assert p.rule == OK and not p.sliced and not p.new_session
    assert (p.slots, p.wgs) == (slots, slots), "every workgroup of an unsliced launch owns one slot"
    assert p.ws_bytes == slots * slot_bytes(380)


def test_slots_are_halved_while_they_claim_more_than_half_of_the_memory():
    s = slot_bytes(380)
    p = sim.plan(sim.facts(total_mem=4 * s), YUD)            # 2 slots fit: 102 -> 51 -> 25 -> 12 -> 6 -> 3 -> 1
    assert (p.rule, p.slots, p.wgs) == (OK, 1, 1)
    assert sim.plan(sim.facts(total_mem=24 * s), YUD).slots == 12     # ... and 12 of them stop at 12
    assert sim.plan(sim.facts(total_mem=24 * s - 2), YUD).slots == 6
    assert sim.plan(sim.facts(total_mem=2 * 102 * s), YUD).slots == 102, "exactly half of the memory: no halving"
    assert sim.plan(sim.facts(total_mem=2 * 102 * s - 2), YUD).slots == 51
    assert sim.plan(sim.facts(total_mem=2 * 102 * s - 1), YUD).slots == 51, "half of an odd size is rounded down"


def test_a_slot_beyond_half_of_the_memory_still_gets_one_slot():
    s = slot_bytes(380)
    for batch in (1, 102):
        p = sim.plan(sim.facts(total_mem=s), [380] * batch)
        assert (p.rule, p.slots, p.wgs, p.ws_bytes) == (OK, 1, 1, s)


def test_workspace_bytes_is_the_unsliced_plan():
    for batch, n_max, slots in ((3, 12, 3), (300, 380, 256)):
        w = sim.workspace(sim.facts(), batch, n_max)
        assert (w.slots, w.ws_bytes) == (slots, slots * slot_bytes(n_max))
    # ... of a handle with a time slice set and images parked, too: vpk_em_workspace_bytes ignores both
    f = sim.facts(slice_ms=5.0, slice_nmax=1000)
    f = sim.with_session(f, sim.plan(f, [12] * 3))
    w = sim.workspace(f, 3, 12)
    assert (w.rule, w.slots, w.ws_bytes) == (OK, 3, 3 * slot_bytes(12))
    p = sim.default_params()
    assert sim.workspace(sim.facts(), 3, 12, p, n_init=3).mcap == 16, "n_init > 0 counts as initial VPs given: 3 + 9 splits"


# ---- sliced -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap, wgs", [(0, 256), (24, 24), (1000, 256)])
def test_sliced_workgroups_do_not_follow_the_batch(cap, wgs):
    for batch in (1, 300):
        p = sim.plan(sim.facts(cap=cap, slice_ms=5.0), [12] * batch)
        assert p.rule == OK and p.sliced and p.new_session
        assert (p.wgs, p.slots) == (wgs, 2 * wgs + 8)
        assert p.ws_bytes == (2 * wgs + 8) * slot_bytes(12)


def test_sliced_slots_are_sized_for_slice_nmax():
    sizes = [12, 40]
    assert sim.plan(sim.facts(slice_ms=5.0, slice_nmax=100), sizes).L.ldn == 104      # above the largest image
    assert sim.plan(sim.facts(slice_ms=5.0, slice_nmax=100), sizes).slot_bytes == slot_bytes(100)
    assert sim.plan(sim.facts(slice_ms=5.0, slice_nmax=20), sizes).L.ldn == 40        # below it
    assert sim.plan(sim.facts(slice_ms=0.0, slice_nmax=100), sizes).L.ldn == 40, "an unsliced launch ignores it"


def test_sliced_slots_beyond_half_of_the_memory_are_refused():
    s = slot_bytes(12)
    assert sim.plan(sim.facts(slice_ms=5.0, total_mem=2 * 520 * s), [12]).rule == OK
    assert refused(sim.plan(sim.facts(slice_ms=5.0, total_mem=2 * 520 * s - 2), [12]), SLICE_MEM)
    assert sim.plan(sim.facts(slice_ms=5.0, total_mem=2 * 56 * s, cap=24), [12]).rule == OK
    assert refused(sim.plan(sim.facts(slice_ms=5.0, total_mem=2 * 56 * s - 2, cap=24), [12]), SLICE_MEM)


def _parked():
    f = sim.facts(slice_ms=5.0, slice_nmax=40, cap=24)
    first = sim.plan(f, [12, 40])
    assert first.rule == OK and first.new_session
    return sim.with_session(f, first), first


def test_the_same_geometry_joins_the_live_session():
    f, first = _parked()
    p = sim.plan(f, [30] * 7)
    assert p.rule == OK and not p.new_session and (p.slots, p.wgs, p.slot_bytes) == (first.slots, first.wgs, first.slot_bytes)


@pytest.mark.parametrize("fact", ["has_sess", "sess_slot_bytes", "sess_slots", "sess_wgs", "layout"])
def test_each_session_fact_alone_makes_a_new_session(fact):
    for unflushed in (True, False):
        f, first = _parked()
        f.unflushed = unflushed
        if fact == "layout":
            f.sess_layout.part += 8                          # one region moved: slot bytes, slots and workgroups the same
        elif fact == "has_sess":
            f.has_sess = False
        else:
            setattr(f, fact, getattr(f, fact) + 1)
        p = sim.plan(f, [12, 40])
        if unflushed:
            assert refused(p, SESS_CHANGED), "parked images were laid out with the old geometry"
        else:
            assert p.rule == OK and p.new_session


def test_a_call_that_changes_the_geometry_is_refused_while_images_are_parked():
    f, _ = _parked()
    assert refused(sim.plan(f, [12, 41]), SESS_CHANGED)                              # more lines than the slots hold
    assert refused(sim.plan(f, [12, 40], sim.default_params(do_split=0)), SESS_CHANGED)
    f.max_workgroups = 23
    assert refused(sim.plan(f, [12, 40]), SESS_CHANGED)
    f.unflushed = False
    assert sim.plan(f, [12, 41]).new_session and sim.plan(f, [12, 41]).rule == OK


def test_the_workspace_must_not_move_while_images_are_parked():
    f, first = _parked()
    f.ws_bytes = first.ws_bytes - 1
    assert refused(sim.plan(f, [12, 40]), WS_MOVES)
    f.ws_bytes = first.ws_bytes
    assert sim.plan(f, [12, 40]).rule == OK
    f.ws_bytes, f.unflushed = 0, False
    assert sim.plan(f, [12, 40]).rule == OK, "nothing parked: the workspace may grow"


def test_the_memory_limit_comes_before_the_session_refusals():
    f, first = _parked()
    f.total_mem, f.sess_slots, f.ws_bytes = 2 * first.ws_bytes - 2, first.slots + 1, 0
    assert refused(sim.plan(f, [12, 40]), SLICE_MEM)
    f.total_mem = 2 * first.ws_bytes
    assert refused(sim.plan(f, [12, 40]), SESS_CHANGED), "a changed layout before a workspace that would move"


def test_an_unsliced_call_with_parked_images_plans_as_after_a_flush():
    f, first = _parked()
    f.slice_ms, f.ws_bytes = 0.0, 0                          # the time slice switched off, the driver flushes before it reserves
    p = sim.plan(f, [12, 41] * 20)
    assert p.rule == OK and not p.sliced and not p.new_session
    assert (p.slots, p.wgs, p.L.ldn) == (24, 24, 48)


# ---- limits -----------------------------------------------------------------------------------------------------------------
def test_line_limit():
    assert sim.plan(sim.facts(), [12, 46000]).rule == OK
    assert refused(sim.plan(sim.facts(), [12, 46001]), LINES)
    assert refused(sim.plan(sim.facts(slice_ms=5.0), [46001, 12]), LINES)


def test_offsets_must_not_decrease():
    assert refused(sim.plan(sim.facts(), [0] * 3, offsets=[0, 12, 24, 20]), OFFSETS)       # at the last image only
    assert refused(sim.plan(sim.facts(), [0] * 3, offsets=[5, 4, 24, 30]), OFFSETS)
    assert sim.plan(sim.facts(), [0] * 3, offsets=[7, 12, 12, 20]).rule == OK, "a window of a longer array, an empty image"


@pytest.mark.parametrize("kw, rule", [({"num_iter": 0}, NUM_ITER), ({"num_iter": 100001}, NUM_ITER), ({"num_iter": 1}, OK),
                                      ({"num_iter": 100000}, OK), ({"split_merge_freq": 0}, FREQ), ({"split_merge_freq": 1}, OK),
                                      ({"num_init_vp": 0}, NUM_INIT), ({"num_init_vp": 65}, NUM_INIT), ({"num_init_vp": 64}, OK),
                                      ({"num_init_vp": 1}, OK)])
def test_parameter_limits(kw, rule):
    assert refused(sim.plan(sim.facts(), [12], sim.default_params(**kw)), rule)


@pytest.mark.parametrize("n_init", [0, 65, 1, 64])
def test_n_init_counts_only_with_initial_vps(n_init):
    bad = n_init in (0, 65)
    assert refused(sim.plan(sim.facts(), [12], n_init=n_init, has_init=True), N_INIT if bad else OK)
    assert sim.plan(sim.facts(), [12], n_init=n_init, has_init=False).rule == OK


def test_arguments_in_the_drivers_order():
    f = sim.facts()
    assert refused(sim.plan(f, [12], buffers=False), NULL)
    assert refused(sim.plan(f, [], offsets=[0]), NULL)                               # batch 0
    assert refused(sim.plan(f, [12], offsets=False), NULL)                           # offsets null
    assert refused(sim.plan(f, [12], sphere_size=19), SPHERE) and sim.plan(f, [12], sphere_size=20).rule == OK
    assert refused(sim.plan(f, [12], max_vp=0), SPHERE) and sim.plan(f, [12], max_vp=1).rule == OK
    assert refused(sim.plan(f, [12], params=False), PARAMS)                          # params null
    bad = sim.default_params(num_iter=0, split_merge_freq=0, num_init_vp=0)
    dec = dict(offsets=[0, 50000, 20])                       # not monotone, and 50000 lines
    assert refused(sim.plan(f, [0, 0], bad, buffers=False, sphere_size=19, n_init=0, has_init=True, **dec), NULL)
    assert refused(sim.plan(f, [0, 0], bad, sphere_size=19, n_init=0, has_init=True, **dec), SPHERE)
    assert refused(sim.plan(f, [0, 0], False, n_init=0, has_init=True, **dec), PARAMS)
    assert refused(sim.plan(f, [0, 0], bad, n_init=0, has_init=True, **dec), NUM_ITER)
    bad.num_iter = 1
    assert refused(sim.plan(f, [0, 0], bad, n_init=0, has_init=True, **dec), FREQ)
    bad.split_merge_freq = 1
    assert refused(sim.plan(f, [0, 0], bad, n_init=0, has_init=True, **dec), NUM_INIT)
    bad.num_init_vp = 1
    assert refused(sim.plan(f, [0, 0], bad, n_init=0, has_init=True, **dec), N_INIT)
    assert refused(sim.plan(f, [0, 0], bad, **dec), OFFSETS)
    assert refused(sim.plan(f, [0, 0], bad, offsets=[0, 50000, 50000]), LINES)
    s = sim.facts(slice_ms=5.0, total_mem=1 << 20)
    assert refused(sim.plan(s, [0, 0], bad, offsets=[0, 50000, 50000]), LINES), "the line limit before the memory limit"


def test_codes_cover_every_rule():
    assert sorted(CODE) == list(range(13))


# ---- mcap, LDS mode -------------------------------------------------------------------------------------------------------
def test_mcap_is_em_layouts():
    assert sim.plan(sim.facts(), [12]).mcap == 40                                    # 25 + 9 splits = 34, rounded up to 8
    assert sim.plan(sim.facts(), [12], sim.default_params(split_merge_freq=1)).mcap == 64      # 25 + 99, clamped to 64
    assert sim.plan(sim.facts(), [12], sim.default_params(do_split=0)).mcap == 32
    assert sim.plan(sim.facts(), [12], n_init=3, has_init=True).mcap == 16           # 3 + 9
    assert sim.plan(sim.facts(), [12]).L.mcap == 40 and sim.plan(sim.facts(), [12]).L.nwaves == 8


def test_lds_mode():
    big = sim.plan(sim.facts(), [12])
    assert big.per_cu == 1 and big.wt_doubles % 32 == 0 and big.lds_bytes <= 163840 < big.lds_bytes + 32 * 8
    shared = big.lds_bytes - 8 * big.wt_doubles              # the Shared block in front of the panel
    for doubles, wt, panel in ((4096, 4096, 4096), (10, 64, 2048), (2048, 2048, 2048), (1 << 30, big.wt_doubles, big.wt_doubles)):
        p = sim.plan(sim.facts(lds_doubles=doubles), [12])   # the launch gets at least the setup phases' 2048 doubles
        assert (p.per_cu, p.wt_doubles, p.lds_bytes) == (1, wt, shared + 8 * panel)


# ---- header ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch, off_bytes, ord_bytes", [(1, 256, 256), (31, 256, 256), (32, 512, 256), (64, 768, 256),
                                                         (65, 768, 512), (97, 1024, 512)])
def test_header_layout(batch, off_bytes, ord_bytes):
    p = sim.plan(sim.facts(), [12] * batch)
    assert (p.off_bytes, p.ord_bytes, p.staged_bytes) == (off_bytes, ord_bytes, off_bytes + ord_bytes)
    assert off_bytes >= 8 * (batch + 1) and ord_bytes >= 4 * batch


def test_order_is_largest_first_and_stable():
    assert sim.order([5, 9, 5, 0, 9, 12, 0]) == [5, 1, 4, 0, 2, 3, 6], "ties in index order, empty images last"
    assert sim.order([7]) == [0] and sim.order([3, 3, 3]) == [0, 1, 2] and sim.order([1, 2, 3]) == [2, 1, 0]
    assert sim.plan(sim.facts(), [5, 0, 0]).rule == OK, "images without lines are allowed"


# ---- session layout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("started_cap, wait_cap", [(1024, 8192), (3, 2), (1, 1)])
@pytest.mark.parametrize("slots", [1, 56, 64, 65, 520])
@pytest.mark.parametrize("carry", [8, 600, 1000])
def test_session_layout(slots, started_cap, wait_cap, carry):
    offs, total = sim.sess_layout(slots, started_cap, wait_cap, carry)
    sizes = [6 * 4, slots * 4, carry * started_cap, carry * started_cap, carry * wait_cap, carry * wait_cap]
    assert offs[0] == 0 and offs[1] == 256, "counters, then the slot flags"
    assert all(o % 256 == 0 for o in offs)
    for k in range(5):
        assert offs[k] + sizes[k] <= offs[k + 1] < offs[k] + sizes[k] + 256, "regions follow each other without overlap"
    assert total == 256 + sum(align(s, 256) for s in sizes[1:]) == offs[5] + align(sizes[5], 256)


def test_slice_budget_in_ticks():
    assert sim.slice_ticks(0.0) == 0, "no deadline"
    assert sim.slice_ticks(1e-9) == 1, "a positive slice is at least one tick"
    for ms in (1.0, 2.5, 40.0):                              # 100 MHz ticks: slice_ms x 1e5, truncated
        assert abs(sim.slice_ticks(ms) - ms * 1e5) <= 1
