"""ctypes access to the TEST-ONLY host build of csrc/em_plan.hpp (tests/hostsim/sim_em_plan.cpp): what vpk_em_batch decides on
the host before it launches.  A library of its own, built by hostbuild.py on first use."""
import ctypes

import numpy as np

from . import hostbuild
from .simlib import EmParams

_Z, _I, _U = ctypes.c_size_t, ctypes.c_int, ctypes.c_ulonglong


class EmLayout(ctypes.Structure):                                # csrc/em_layout.hpp
    _fields_ = [(n, _I) for n in ("ldn", "ld", "mcap", "nwaves")] + \
               [(n, _Z) for n in ("lsim", "pdist", "den", "lweight", "langle", "lscore", "rowsum", "lvsq", "pvl", "w", "wsrc", "drow",
                                  "part", "cl", "assoc", "idx", "lcopy", "lpcopy", "state", "total_doubles")]


class EmFacts(ctypes.Structure):                                 # csrc/em_plan.hpp
    _fields_ = [("cu_share", _I), ("max_workgroups", _I), ("total_mem", _Z), ("lds_doubles", _I), ("slice_ms", ctypes.c_double),
                ("slice_nmax", _I), ("started_cap", _I), ("wait_cap", _I), ("has_sess", ctypes.c_bool), ("sess_slot_bytes", _Z),
                ("sess_slots", _I), ("sess_wgs", _I), ("sess_layout", EmLayout), ("unflushed", ctypes.c_bool), ("ws_bytes", _Z)]


class Plan(ctypes.Structure):                                    # sim_em_plan.cpp: SimEmPlan
    _fields_ = [(n, _I) for n in ("rule", "code", "sliced", "mcap", "slots", "wgs", "new_session", "per_cu", "wt_doubles")] + \
               [(n, _U) for n in ("slot_bytes", "ws_bytes", "off_bytes", "ord_bytes", "staged_bytes", "lds_bytes")] + [("L", EmLayout)]


_lib = None


def default_params(**kw):
    """vpk_em_default_params (csrc/vpk_core.hip), written out"""
    p = EmParams(num_iter=100, do_merge=1, do_split=1, do_iterations=1, use_weights=1, num_init_vp=25, split_merge_freq=10,
                 num_min_lines=3, wbias=1.0, merge_thresh=1e-3, outlier_thresh=1.96 * 1.96, final_convergence=5e-3, s_thresh=1e-200)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def lib():
    global _lib
    if _lib is None:
        _lib = hostbuild.load("em_plan")
        sizes = (ctypes.c_int * 4)()
        _lib.sim_em_plan_sizes(sizes)
        assert list(sizes) == [ctypes.sizeof(EmFacts), ctypes.sizeof(EmLayout), ctypes.sizeof(Plan), ctypes.sizeof(EmParams)]
        _lib.sim_em_slice_ticks.restype = ctypes.c_longlong
        _lib.sim_em_slice_ticks.argtypes = [ctypes.c_double]
        _lib.sim_em_sess_layout.argtypes = [_I, _I, _I, _U, ctypes.c_void_p]
    return _lib


def facts(cu_share=256, cap=0, total_mem=288 << 30, lds_doubles=0, slice_ms=0.0, slice_nmax=0, started_cap=1024, wait_cap=8192):
    """the facts of a handle without a session"""
    return EmFacts(cu_share=cu_share, max_workgroups=cap, total_mem=total_mem, lds_doubles=lds_doubles, slice_ms=slice_ms,
                   slice_nmax=slice_nmax, started_cap=started_cap, wait_cap=wait_cap)


def with_session(f, plan, unflushed=True, ws_bytes=None):
    """f after a sliced call that planned as `plan`: a live session with parked images, the workspace the call reserved"""
    g = EmFacts.from_buffer_copy(f)
    g.has_sess, g.sess_slot_bytes, g.sess_slots, g.sess_wgs = True, plan.slot_bytes, plan.slots, plan.wgs
    g.sess_layout = EmLayout.from_buffer_copy(plan.L)
    g.unflushed, g.ws_bytes = unflushed, plan.ws_bytes if ws_bytes is None else ws_bytes
    return g


def plan(f, sizes, params=None, buffers=True, sphere_size=500, max_vp=64, n_init=0, has_init=False, offsets=None):
    """em_plan for a batch of len(sizes) images with `sizes` lines, or with explicit offsets (False: a null pointer);
    params False: a null pointer"""
    batch = len(sizes)
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum(np.asarray(sizes, dtype=np.int64))))
    off = None if offsets is False else np.ascontiguousarray(offsets, dtype=np.int64)
    p = default_params() if params is None else params
    out = Plan()
    rule = lib().sim_em_plan(ctypes.byref(f), batch, None if off is None else off.ctypes.data_as(ctypes.c_void_p), int(buffers),
                             sphere_size, max_vp, None if p is False else ctypes.byref(p), n_init, int(has_init), ctypes.byref(out))
    assert rule == out.rule
    return out


def workspace(f, batch, n_max, params=None, n_init=0):
    """the plan behind vpk_em_workspace_bytes"""
    p = default_params() if params is None else params
    out = Plan()
    lib().sim_em_workspace(ctypes.byref(f), batch, n_max, ctypes.byref(p), n_init, ctypes.byref(out))
    return out


def order(sizes):
    off = np.concatenate(([0], np.cumsum(np.asarray(sizes, dtype=np.int64))))
    o = np.full(len(sizes), -7, np.int32)
    lib().sim_em_order(len(sizes), off.ctypes.data_as(ctypes.c_void_p), o.ctypes.data_as(ctypes.c_void_p))
    return o.tolist()


def sess_layout(slots, started_cap, wait_cap, carry_bytes):
    """byte offsets (head, busy, started A, B, waiting A, B) and the total"""
    out = (_U * 7)()
    lib().sim_em_sess_layout(slots, started_cap, wait_cap, carry_bytes, out)
    return list(out[:6]), out[6]


def slice_ticks(slice_ms):
    return lib().sim_em_slice_ticks(slice_ms)
