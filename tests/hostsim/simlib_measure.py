"""ctypes access to the TEST-ONLY host build of em_run<MEASURE> (tests/hostsim/sim_em_measure.cpp): the EM driver on one
image under "angle" or "dotprod".  A library of its own, built by hostbuild.py on first use; simlib.py's stays as it is."""
import ctypes

import numpy as np

from . import hostbuild, simlib

MEASURES = {"angle": 0, "dotprod": 1}       # include/vpk.h: VPK_DIST_ANGLE, VPK_DIST_DOTPROD


def lib():
    return hostbuild.load("measure")


def em_single(l, lp, cnn, sphere, distance_measure="dotprod", init_vp=None, max_vp=64, sliced=False, lds_doubles=None,
              want_distribution=False, **kw):
    """simlib.em_single's result (without states, trace and metric) from em_run<MEASURE>; want_distribution adds the last
    E-step's "lvsq" (N, M) and "p_vl" (M, N)."""
    n = lp.shape[0]
    p = simlib.default_params(**kw)
    l = np.ascontiguousarray(l, dtype=np.float64)
    lp = np.ascontiguousarray(lp, dtype=np.float64)
    cnn = np.ascontiguousarray(cnn, dtype=np.float32)
    sphere = np.ascontiguousarray(sphere, dtype=np.uint8)
    iv = np.ascontiguousarray(init_vp, dtype=np.float64) if init_vp is not None else None
    vp = np.zeros((max_vp, 3)); sigma = np.zeros(max_vp); counts = np.zeros(max_vp); cw = np.zeros(max_vp)
    num = np.zeros(1, np.int32); assoc = np.zeros(n, np.int64); it = np.zeros(1, np.int32)
    st = np.zeros(1, np.int32); fl = np.zeros(1, np.uint32)
    lvsq = np.zeros((n, max_vp)) if want_distribution else None
    pvl = np.zeros((n, max_vp)) if want_distribution else None
    D, I, L, U, P = ctypes.c_double, ctypes.c_int32, ctypes.c_longlong, ctypes.c_uint32, simlib._p
    slices = lib().sim_em_measure(MEASURES[distance_measure], int(bool(sliced)), int(lds_doubles or 0), n, P(l, D), P(lp, D),
                                  P(cnn, ctypes.c_float), P(sphere, ctypes.c_ubyte), sphere.shape[0], P(iv, D),
                                  0 if iv is None else iv.shape[0], ctypes.byref(p), max_vp, P(vp, D), P(sigma, D),
                                  P(counts, D), P(cw, D), P(num, I), P(assoc, L), P(it, I), P(st, I), P(fl, U), P(lvsq, D),
                                  P(pvl, D))
    assert slices >= 0
    m = int(num[0])
    res = {"slices": slices, "status": int(st[0]), "flags": int(fl[0]), "iterations": int(it[0]), "vp": vp[:m],
           "sigma": sigma[:m], "counts": counts[:m], "counts_weighted": cw[:m], "vp_assoc": assoc, "l": l}
    if want_distribution:
        res["lvsq"] = lvsq[:, :m].copy()
        res["p_vl"] = pvl[:, :m].T.copy()
    return res
