"""The recorded runs of the REFERENCE's expectation_maximisation under distance_measure="dotprod" (tests/golden/em_dotprod/,
written by scripts/make_em_dotprod_goldens.py), shared by tests/test_em_dotprod.py (CPU: the host build of em_run<MEASURE>)
and tests/test_gpu_em_dotprod.py (the kernel).

A file ``<case>.npz`` holds the reference's result on the inputs and keywords of tests/golden/<case>.npz; a file
``<case>__<variant>.npz`` carries keywords of its own (``kw_*``, ``init_vp``, or ``drop_init_vp``: run without the stored
init_vp) that are laid over the stored ones.  Every file was written only after the reference gave the same iterations, VP
count and assignments on the stored inputs and on two one-ulp nudges of them, so the bar is golden_util.check_em_result's
(assignments, counts and iterations equal, VPs and sigma 1e-4, weighted counts 1e-9) without a certificate."""
import os

import numpy as np

from conftest import GOLDEN
from golden_util import em_kwargs, load

DIR = os.path.join(GOLDEN, "em_dotprod")


def stems():
    return sorted(f[:-4] for f in os.listdir(DIR) if f.endswith(".npz"))


_cache = {}


def case(stem):
    """(inputs of tests/golden/<case>.npz, keywords of the run without distance_measure, the recorded result).  Read once;
    nobody writes into what this returns."""
    if stem not in _cache:
        g = load(stem.split("__")[0])
        r = dict(np.load(os.path.join(DIR, stem + ".npz"), allow_pickle=False))
        kw = em_kwargs(g)
        for k in r:
            if k.startswith("kw_"):
                kw[k[3:]] = r[k].item()
        if "init_vp" in r:
            kw["init_vp"] = r["init_vp"]
        if "drop_init_vp" in r:
            kw.pop("init_vp", None)
        _cache[stem] = (g, kw, r)
    return _cache[stem]


def scene(stem):
    """em.em_batch's scene of a case (a fresh ``l``: the EM normalises it in place) and the keywords that are not in it."""
    g, kw, _ = case(stem)
    kw = dict(kw)
    init = kw.pop("init_vp", None)
    return {"l": g["l"].copy(), "lp": g["lp"], "cnn_response": g["cnn_response"], "sphere_image": g["sphere_image"],
            "init_vp": init}, kw


def same_bits(a, b, keys=("vp", "sigma", "counts", "counts_weighted", "vp_assoc")):
    assert a["status"] == b["status"] and a["iterations"] == b["iterations"]
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# The last E-step against the recording.  The kernel's VPs and variances are not the reference's to the bit, so its lvsq
# and p_vl cannot be either; what is asked is agreement FIVE orders inside the parity bar: VPs within VP_DELTA = 1e-9
# (absolute, unit vectors) and variances within S_DELTA = 1e-9 relative of the recorded ones.  Every recorded case is one on
# which the reference itself moves by at most 3.5e-14 under one-ulp input changes (the files' vp_spread), so nothing but
# rounding separates two correct fp64 evaluations there.  From those two figures, and from nothing the code returns:
#   lvsq = lv^2, lv = l . v with |l| = 1: |d lv| <= VP_DELTA, so |d lvsq| <= (2 |lv| + VP_DELTA) VP_DELTA, plus the fp64
#       rounding of the two evaluations, 8 u lvsq + 8 u |lv| at most (estep_reference.lvsq_dotprod: 3 u sum |l_i v_i| <= 3 sqrt(3) u).
#   p_vl = softmax over the VPs of -a_m + log(k2_m p_v_m), a = lvsq / (2 s): |d p_vl| <= max |d a_m| / 2 over the VPs whose
#       term is not negligible.  A line that is not on the 1e-12 floor of p_l has a term of at least 1e-12 / 64, and
#       k2 p_v <= 1e5 at the variances seen here, so its smallest a is below 45; a term more than 50 above that is below 1e-17
#       of it.  So a <= 100 where it matters, and there d a = a (d lvsq / lvsq + S_DELTA) <= 100 S_DELTA + |lv| VP_DELTA / s
#       <= 100 S_DELTA + sqrt(200 / s_min) VP_DELTA.  Lines on the floor (sum_m p_vl < 1 - 1e-6 in the recording) divide
#       by the constant instead: there d p_vl / p_vl <= d a, and p_vl <= 1.
VP_DELTA = 1e-9
S_DELTA = 1e-9
U = 2.0 ** -53


def check_last_estep(vp, sigma, lvsq, p_vl, r):
    """vp (M, 3), sigma (M), lvsq (N, M), p_vl (M, N) of a run against the recording r; returns the worst error / tolerance."""
    assert np.abs(vp - r["o_vp"]).max() <= VP_DELTA
    assert np.abs(sigma / r["o_sigma"] - 1).max() <= S_DELTA
    lv = np.sqrt(r["d_lvsq"])
    tol_lvsq = (2 * lv + VP_DELTA) * VP_DELTA + 8 * U * (r["d_lvsq"] + lv)
    e_lvsq = np.abs(lvsq - r["d_lvsq"]) / tol_lvsq
    da = 100 * S_DELTA + np.sqrt(200 / r["o_sigma"].min()) * VP_DELTA
    e_pvl = np.abs(p_vl - r["d_p_vl"]) / da            # (da / 2 off the floor, da on it: the looser one for both)
    assert e_lvsq.max() <= 1.0, ("lvsq", float(e_lvsq.max()))
    assert e_pvl.max() <= 1.0, ("p_vl", float(e_pvl.max()), da)
    return float(e_lvsq.max()), float(e_pvl.max())
