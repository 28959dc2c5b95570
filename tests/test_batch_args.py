"""csrc/batch_args.hpp -- the rules the batch drivers (vpk_vpset.hip, vpk_emstep.hip, vpk_estep.hip, vpk_lines.hip) hold their
host offsets to -- compiled for the host by tests/hostsim/sim_batch_args.cpp, each rule at its edge.  CPU only."""
import ctypes

import numpy as np
import pytest

from hostsim import hostbuild

OK, EMPTY, NEGATIVE, NULL, OFFSETS, VPS, LINES, SLOT = range(8)      # BatchRule
VPK_OK, VPK_ERR_ARG, VPK_ERR_LIMIT = 0, -1, -5                       # include/vpk.h
MAX_VP, MAX_LINES = 64, 32768                                        # what vpk_vpset.hip and vpk_emstep.hip pass
LP = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def sim():
    lib = hostbuild.load("batch_args")
    lib.sim_batch_offsets.argtypes = [ctypes.c_int, LP, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
    lib.sim_batch_pair.argtypes = [ctypes.c_int, LP, LP, ctypes.c_longlong, ctypes.c_longlong]
    lib.sim_batch_slots.argtypes = [ctypes.c_int, LP, LP]
    return lib


def _p(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(LP)


def offsets(sim, off, index_max=-1):
    largest = ctypes.c_longlong(-7)
    return sim.sim_batch_offsets(len(off) - 1, _p(off), index_max, ctypes.byref(largest)), largest.value


def pair(sim, lo, vo, batch=None, max_lines=MAX_LINES, max_vps=MAX_VP):
    return sim.sim_batch_pair(len(lo) - 1 if batch is None else batch, _p(lo), _p(vo), max_lines, max_vps)


def test_offsets_rise_from_a_value_that_is_not_negative(sim):
    assert offsets(sim, [0, 5, 5, 8]) == (OK, 5)
    assert offsets(sim, [3, 4]) == (OK, 1), "a batch may be a window of longer arrays"
    assert offsets(sim, [0]) == (OK, 0)
    assert offsets(sim, [-1, 4])[0] == OFFSETS
    assert offsets(sim, [0, 5, 4, 8])[0] == OFFSETS, "one step down"
    # vpk_lines.hip also bounds every image by what its kernels index with ints
    lim = 0x7fffffff // 4
    assert offsets(sim, [0, lim], lim) == (OK, lim) and offsets(sim, [0, lim + 1], lim)[0] == OFFSETS
    assert offsets(sim, [0, lim + 1]) == (OK, lim + 1)


def test_pair_reports_in_the_drivers_order(sim):
    lo, vo = [0, 5, 5, 8], [0, 2, 3, 3]
    assert pair(sim, lo, vo) == OK
    assert pair(sim, lo, vo, batch=0) == EMPTY and pair(sim, None, None, batch=0) == EMPTY
    assert pair(sim, lo, vo, batch=-1) == NEGATIVE and pair(sim, None, None, batch=-1) == NEGATIVE
    assert pair(sim, None, vo, batch=3) == NULL and pair(sim, lo, None, batch=3) == NULL
    assert pair(sim, [-1, 5, 5, 8], vo) == OFFSETS and pair(sim, lo, [-1, 2, 3, 3]) == OFFSETS
    assert pair(sim, [0, 5, 4, 8], vo) == OFFSETS and pair(sim, lo, [0, 2, 1, 3]) == OFFSETS
    # malformed offsets are reported before a limit, too many VPs before too many lines
    assert pair(sim, [0, MAX_LINES + 1, 0], [0, MAX_VP + 1, 0], batch=2) == OFFSETS
    assert pair(sim, [0, MAX_LINES + 1], [0, MAX_VP + 1]) == VPS


def test_limits_at_their_edges(sim):
    assert pair(sim, [0, 1, 2], [0, MAX_VP, 2 * MAX_VP]) == OK
    assert pair(sim, [0, 1, 2], [0, MAX_VP, 2 * MAX_VP + 1]) == VPS
    assert pair(sim, [0, MAX_LINES, 2 * MAX_LINES], [0, 1, 2]) == OK
    assert pair(sim, [0, MAX_LINES, 2 * MAX_LINES + 1], [0, 1, 2]) == LINES
    # vpk_estep.hip passes no limit: any N_b, any M_b
    assert pair(sim, [0, MAX_LINES + 1], [0, MAX_VP + 1], max_lines=-1, max_vps=-1) == OK


def test_matrix_slots(sim):
    off = [0, 5, 5, 8]                                               # N = 5, 0, 3
    assert sim.sim_batch_slots(3, _p(off), _p([0, 25, 25, 34])) == OK
    assert sim.sim_batch_slots(3, _p(off), _p([0, 32, 32, 48])) == OK, "gaps between the slots (calc_lsim_batch aligns them)"
    assert sim.sim_batch_slots(3, _p(off), _p([0, 24, 24, 33])) == SLOT, "N^2 - 1 elements for the first image"
    assert sim.sim_batch_slots(3, _p(off), _p([0, 25, 25, 33])) == SLOT, "N^2 - 1 elements for the last"
    assert sim.sim_batch_slots(3, _p(off), _p([-1, 25, 25, 34])) == SLOT
    assert sim.sim_batch_slots(3, _p(off), _p([0, 25, 24, 34])) == SLOT, "an empty image's slot may not step down"
    assert sim.sim_batch_slots(0, _p(off), _p([0])) == OK


def test_codes(sim):
    want = {OK: VPK_OK, EMPTY: VPK_OK, VPS: VPK_ERR_LIMIT, LINES: VPK_ERR_LIMIT}
    for rule in range(8):
        assert sim.sim_batch_code(rule) == want.get(rule, VPK_ERR_ARG)
