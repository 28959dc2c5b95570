"""ctypes access to the TEST-ONLY host build tests/hostsim/sim_em_estep_zeros.cpp: a lone E-step + smoother and the whole EM
on one image, under either measure AND either setting of EmCtx::smoother (0: the E-step's three passes, 1: the dense form).
A library of its own, built by hostbuild.py on first use; simlib.py's stays as it is."""
import ctypes

import numpy as np

from . import hostbuild, simlib

MEASURES = {"angle": 0, "dotprod": 1}       # include/vpk.h: VPK_DIST_ANGLE, VPK_DIST_DOTPROD


def lib():
    return hostbuild.load("estep_zeros")


def estep_smooth(l, lp, cnn, v, s, lweight, lsim, measure="angle", smoother=0, lds_doubles=None, bias=1.0):
    """{"p_v" (M), "lvsq" (M, N), "p_vl" (M, N), "w" (M, N), "s" (M, floored), "plan", "panel_flag"}"""
    n, m = lp.shape[0], v.shape[0]
    D, P = ctypes.c_double, simlib._p
    l, lp, v, lweight, lsim = (np.ascontiguousarray(a, dtype=np.float64) for a in (l, lp, v, lweight, lsim))
    cnn = np.ascontiguousarray(cnn, dtype=np.float32)
    s = np.ascontiguousarray(s, dtype=np.float64).copy()
    pv = np.zeros(m); lvsq = np.zeros((m, n)); pvl = np.zeros((m, n)); w = np.zeros((m, n)); info = np.zeros(2, np.int32)
    rc = lib().sim_estep_zeros(MEASURES[measure], int(smoother), int(lds_doubles or 0), n, m, P(l, D), P(lp, D),
                               P(cnn, ctypes.c_float), P(v, D), P(s, D), P(lweight, D), P(lsim, D), D(bias), P(pv, D),
                               P(lvsq, D), P(pvl, D), P(w, D), P(info, ctypes.c_int32))
    assert rc == 0
    return {"p_v": pv, "lvsq": lvsq, "p_vl": pvl, "w": w, "s": s, "plan": int(info[0]), "panel_flag": int(info[1])}


def em_single(l, lp, cnn, sphere, distance_measure="angle", smoother=0, init_vp=None, max_vp=64, lds_doubles=None, **kw):
    """simlib_measure.em_single's result, with the last E-step's "lvsq" (N, M) and "p_vl" (M, N), under EmCtx::smoother"""
    n = lp.shape[0]
    p = simlib.default_params(**kw)
    l = np.ascontiguousarray(l, dtype=np.float64).copy()
    lp = np.ascontiguousarray(lp, dtype=np.float64)
    cnn = np.ascontiguousarray(cnn, dtype=np.float32)
    sphere = np.ascontiguousarray(sphere, dtype=np.uint8)
    iv = np.ascontiguousarray(init_vp, dtype=np.float64) if init_vp is not None else None
    vp = np.zeros((max_vp, 3)); sigma = np.zeros(max_vp); counts = np.zeros(max_vp); cw = np.zeros(max_vp)
    num = np.zeros(1, np.int32); assoc = np.zeros(n, np.int64); it = np.zeros(1, np.int32)
    st = np.zeros(1, np.int32); fl = np.zeros(1, np.uint32)
    lvsq = np.zeros((n, max_vp)); pvl = np.zeros((n, max_vp))
    D, I, L, U, P = ctypes.c_double, ctypes.c_int32, ctypes.c_longlong, ctypes.c_uint32, simlib._p
    rc = lib().sim_em_zeros(MEASURES[distance_measure], int(smoother), int(lds_doubles or 0), n, P(l, D), P(lp, D),
                            P(cnn, ctypes.c_float), P(sphere, ctypes.c_ubyte), sphere.shape[0], P(iv, D),
                            0 if iv is None else iv.shape[0], ctypes.byref(p), max_vp, P(vp, D), P(sigma, D), P(counts, D),
                            P(cw, D), P(num, I), P(assoc, L), P(it, I), P(st, I), P(fl, U), P(lvsq, D), P(pvl, D))
    assert rc == 0
    m = int(num[0])
    return {"status": int(st[0]), "flags": int(fl[0]), "iterations": int(it[0]), "vp": vp[:m], "sigma": sigma[:m],
            "counts": counts[:m], "counts_weighted": cw[:m], "vp_assoc": assoc, "lvsq": lvsq[:, :m].copy(),
            "p_vl": pvl[:, :m].T.copy()}
