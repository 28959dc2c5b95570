"""ctypes access to the TEST-ONLY host build of vpset_run<MEASURE> (tests/hostsim/sim_vpset.cpp): the stand-alone counts
and merge on one image under "angle", "dotprod" or "area".  A library of its own, built by hostbuild.py on first use."""
import ctypes

import numpy as np

from . import hostbuild, simlib

MEASURES = {"angle": 0, "dotprod": 1, "area": 2}       # include/vpk.h: enum vpk_dist_measure


def lib():
    return hostbuild.load("vpset")


def _c(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def counts(measure, vp, lp, l, s, metric, lweights, thresh=2.57, vp_assoc=None):
    """(counts, counts_weighted, vp_assoc) of one image with lines and VPs"""
    D, L, P = ctypes.c_double, ctypes.c_longlong, simlib._p
    vp, lp, l, s, metric, lw = (_c(x, np.float64) for x in (vp, lp, l, s, metric, lweights))
    ain = _c(vp_assoc, np.int64)
    n, m = lp.shape[0], vp.shape[0]
    c, cw, a = np.zeros(m), np.zeros(m), np.zeros(n, np.int64)
    rc = lib().sim_vpset_counts(MEASURES[measure], n, m, P(lp, D), P(l, D), P(vp, D), P(s, D), P(metric, D), P(lw, D),
                                ctypes.c_double(thresh), P(ain, L), P(c, D), P(cw, D), P(a, L))
    assert rc == 0
    return c, cw, a


def merge(measure, v, s, l, thresh, lw, lsim, wbias, prior_weights, prior_sigma, lp, max_stdd=0.01):
    """(v (M', 3), s (M'), kept (M'), flags) of one image with lines and VPs"""
    D, I, P = ctypes.c_double, ctypes.c_int32, simlib._p
    v, s, l, lw, lsim, lp = (_c(x, np.float64) for x in (v, s, l, lw, lsim, lp))
    pw = _c(prior_weights, np.float32)
    n, m = lp.shape[0], v.shape[0]
    vo, so, keep = np.zeros((m, 3)), np.zeros(m), np.zeros(m, np.int32)
    mo, fl = np.zeros(1, np.int32), np.zeros(1, np.uint32)
    rc = lib().sim_vpset_merge(MEASURES[measure], n, m, P(lp, D), P(l, D), P(v, D), P(s, D), P(lw, D), P(lsim, D),
                               ctypes.c_double(wbias), P(pw, ctypes.c_float), ctypes.c_double(prior_sigma),
                               ctypes.c_double(thresh), ctypes.c_double(max_stdd), P(vo, D), P(so, D), P(mo, I), P(keep, I),
                               P(fl, ctypes.c_uint32))
    assert rc == 0
    k = int(mo[0])
    return vo[:k], so[:k], keep[:k], int(fl[0])
