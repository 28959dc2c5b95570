"""CPU twins of tests/test_gpu_em_phases.py: the same generated inputs (tests/em_phase_reference.py) through

  * the host build of the UNMODIFIED device source (tests/hostsim), under the same bars as the HIP kernels, and
  * the float64 oracle (oracle/em_numpy.py; LAPACK for the null vector) on its own: it must pass every bar and stay inside
    every cap on every input, which shows that no bar is tighter than float64 arithmetic allows and no cap hides a case.

The extended-precision references are computed once per case and shared by both.
"""
import functools

import numpy as np
import pytest

import em_phase_reference as R
from hostsim import simlib
from oracle import em_numpy as em

LD = R.LD


# ---- the reference module's own tools ------------------------------------------------------------------------
def test_jacobi_svd_against_lapack_and_the_cross_product():
    rs = np.random.RandomState(3)
    for n in (3, 4, 17, 200):
        a = rs.randn(n, 3) * np.array([1.0, 0.5, 0.1])       # well conditioned
        sv, v = R.jacobi_svd(a)
        _, sv_np, vt = np.linalg.svd(a, full_matrices=False)
        assert np.abs(sv.astype(np.float64) - sv_np).max() <= 1e-14 * sv_np[0]
        for k in range(3):
            assert min(np.abs(v[:, k].astype(np.float64) - vt[k]).max(), np.abs(v[:, k].astype(np.float64) + vt[k]).max()) <= 1e-13
        assert np.abs((v.T @ v).astype(np.float64) - np.eye(3)).max() <= 1e-18
    for _ in range(20):                                      # two lines: the null vector is their normalised cross product
        l = rs.randn(2, 3)
        r = rs.uniform(0.1, 1, 2)
        ref = R.null_vector_reference(l, r)
        x = np.cross(R.ld(l[0]), R.ld(l[1]))
        x = x / np.sqrt(np.dot(x, x))
        x = x * np.sign(x[2])
        # both sides in extended precision: a few hundred of ITS roundings times the problem's conditioning s1 / s2
        assert float(np.abs(ref["vp"] - x).max()) <= 256 * float(np.finfo(LD).eps) * float(ref["sv"][0] / ref["sv"][1])
        assert ref["sv"][2] <= 1e-17 * ref["sv"][0]          # (three columns in two dimensions: zero to the sweep's tolerance)


def test_shape_lists_meet_the_issue():
    shapes = R.estep_shapes()
    assert {n for n, _ in shapes} == set(R.ESTEP_N) and {m for _, m in shapes} == set(R.ESTEP_M)
    for n in R.ESTEP_N:
        ms = [m for nn, m in shapes if nn == n]
        assert any(m < 8 for m in ms) and any(m % 4 for m in ms) and 32 in ms and 33 in ms
    shapes = R.mstep_shapes()
    assert {n for n, _ in shapes} == set(R.MSTEP_N) and {m for _, m in shapes} == set(R.MSTEP_M)


# ---- shared, cached references -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def estep_setup(n, m):
    case = R.estep_case(n, m)
    par = em.pdf_params(case["cnn"].copy())
    ref = R.estep_reference(par, case["v"], case["lp"], case["s"])
    with np.errstate(all="ignore"):
        orc = em.calc_probabilities(par, case["v"], case["lp"], case["s"].copy())
    return case, ref, orc


@functools.lru_cache(maxsize=None)
def mstep_setup(n, m, hard):
    case = R.mstep_case(n, m, hard)
    ref = R.mstep_reference(case["l"], case["w"], case["lvsq"], case["p_vl"], None, case["assoc"], R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH)
    cur = R.mstep_cur(case, ref, lambda k: k % 12)
    return case, ref, cur


@functools.lru_cache(maxsize=None)
def pairwise_setup(n):
    lp = R.pairwise_case(n)
    ref = R.pairwise_reference(lp)
    with np.errstate(all="ignore"):
        dist = em.pair_distance_closest(lp)
        orc = (em.calc_lsim(lp, sigma=1, dist=dist), em.line_rating_knn(lp, k2=4, dist=dist), em.lines_angles(lp))
    return lp, ref, orc


def oracle_mstep_full(case, cur, hard, max_stdd, s_thresh):
    """oracle/em_numpy.py's soft (lines 632-648 there) and hard (666-683) M-step loops, in the hook's output convention."""
    l, w, lvsq, p_vl, assoc = case["l"], case["w"], case["lvsq"], case["p_vl"], case["assoc"]
    m = w.shape[0]
    vp = np.zeros((m, 3)); s = -np.ones(m); err = -np.ones(m); removed = np.zeros(m, np.int32)
    for k in range(m):
        if hard:
            sel = assoc == k
            if not sel.any():
                continue
            new = em.calc_new_vanishing_point(l[sel], w[k, sel] / np.max(w[k, sel]))
        else:
            new = em.calc_new_vanishing_point(l, w[k])
        if new is None:
            removed[k] = 1
            continue
        vp[k] = new
        sm = np.minimum(em._variance(lvsq[k], p_vl[k]), max_stdd)
        if not hard:
            sm = np.maximum(sm, s_thresh)
        s[k] = sm
        if np.isnan(sm) or (hard and sm < s_thresh):
            removed[k] = 1
        else:
            err[k] = np.arccos(np.minimum(np.abs(np.dot(cur[k], new)), 1.0))
            removed[k] = int(err[k] > 1.5)
    return vp, s, err, removed


# ---- E-step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", R.estep_shapes())
def test_estep_oracle_meets_the_bars(n, m):
    case, ref, orc = estep_setup(n, m)
    R.check_estep({"p_v": orc.v, "lvsq": orc.lvsq, "p_vl": orc.vl, "p_l": orc.l, "s": np.maximum(case["s"], 1e-200)}, case, ref, orc)


@pytest.mark.parametrize("n,m", R.estep_shapes())
def test_estep_host_build(n, m):
    case, ref, orc = estep_setup(n, m)
    pv, lvsq, pvl, s = simlib.estep(case["lp"], case["cnn"], case["v"], case["s"])
    R.check_estep({"p_v": pv, "lvsq": lvsq.T, "p_vl": pvl, "p_l": None, "s": s}, case, ref, orc)


def test_estep_inputs_reach_the_edges():
    """The generated calls contain what the issue lists: NaN lines, the p_l floor, the s floor, an exp that underflows
    beside one that does not, and elements whose bound is finite in (nearly) every call."""
    floor = nan = sfloor = under = 0
    for n, m in R.estep_shapes():
        case, ref, orc = estep_setup(n, m)
        floor += int(np.any(np.asarray(orc.l) == 1e-12))
        nan += int(np.isnan(orc.lvsq).any())
        sfloor += int(np.any(case["s"] < 1e-200))
        under += int(np.any(orc.lv == 0) and np.any(orc.lv > 0))
        if not np.isnan(orc.l).all():
            assert np.isfinite(ref["b_pvl"]).mean() > 0.5
    assert floor >= 3 and nan >= 10 and sfloor >= 10 and under >= 10


# ---- M-step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("n,m", R.mstep_shapes())
def test_mstep_lapack_meets_the_bars(n, m, hard):
    case, ref, cur = mstep_setup(n, m, hard)
    with np.errstate(all="ignore"):
        out = oracle_mstep_full(case, cur, hard, R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH)
    R.check_mstep(out, case, ref, cur, hard)


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("n,m", R.mstep_shapes())
def test_mstep_host_build(n, m, hard):
    case, ref, cur = mstep_setup(n, m, hard)
    out = simlib.mstep_full(case["l"], case["w"], case["lvsq"], case["p_vl"], cur, case["assoc"], R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH)
    R.check_mstep(out, case, ref, cur, hard)


def test_mstep_inputs_reach_the_edges():
    """Tight bundles with s2 / s1 near 1e-2, 1e-4 and 1e-6 whose null vector IS determined (a finite bound), every kind of
    row, both clamps and the removals are among the generated calls."""
    ratios, kinds = [], set()
    for n, m in R.mstep_shapes():
        for hard in (False, True):
            _, ref, _ = mstep_setup(n, m, hard)
            for rec in ref:
                kinds.add(rec["kind"])
                if rec["kind"] == "svd" and np.isfinite(rec["vec_bound"]) and rec["sv"][1] > 0:
                    ratios.append(float(rec["sv"][1] / rec["sv"][0]))
    ratios = np.array(ratios)
    assert kinds == {"skip", "none", "one", "svd"}
    for lo, hi in ((3e-3, 3e-2), (3e-5, 3e-4), (3e-7, 3e-6)):
        assert ((ratios > lo) & (ratios < hi)).sum() >= 5, (lo, hi)


# ---- pairwise ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.PAIR_N)
def test_pairwise_oracle_meets_the_bars(n):
    lp, ref, orc = pairwise_setup(n)
    R.check_pairwise(orc, lp, ref, orc)


@pytest.mark.parametrize("n", R.PAIR_N)
def test_pairwise_host_build(n):
    lp, ref, orc = pairwise_setup(n)
    R.check_pairwise(simlib.pairwise(lp), lp, ref, orc)


# ---- initial VPs ---------------------------------------------------------------------------------------------------
def check_init(got_v0, got_w, cnn, sphere, num_max):
    """Against find_initial_vps / pdf_params: count and order exact, VPs to 1e-13, prior weights bit for bit.  The
    response values are distinct float32 numbers by construction: the order among exactly tied responses is a property
    of NumPy's sort, not of this library, and is not tested."""
    try:
        want = em.find_initial_vps(sphere, cnn, num_max)
    except ValueError:                                        # np.vstack([]): no cell survives
        want = np.zeros((0, 3))
    assert got_v0.shape == want.shape
    if want.size:
        assert np.abs(got_v0 - want).max() <= 1e-13
    assert np.array_equal(got_w, em.pdf_params(cnn.copy()).weights)


@pytest.mark.parametrize("ssize,num_max,kind", R.INIT_CASES)
def test_init_vps_host_build(ssize, num_max, kind):
    cnn, sphere = R.init_case(ssize, num_max, kind)
    assert np.unique(cnn).size == 400 or kind == "few"
    v0, w = simlib.init_vps(cnn, sphere, num_max)
    check_init(v0, w, cnn, sphere, num_max)


# ---- line counts ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counts_setup(n, m):
    case = R.counts_case(n, m)
    par = em.pdf_params(case["cnn"].copy())
    ref = R.estep_reference(par, case["v"], case["lp"], case["s"])
    with np.errstate(all="ignore"):
        orc = em.calc_probabilities(par, case["v"], case["lp"], case["s"].copy())
    metric = np.asarray(orc.vl).copy()                        # a real E-step's p_vl as the decision metric ...
    if m > 1 and n > 3:
        metric[:, 0] = np.nan                                 # ... with a NaN column: np.argmax takes the first NaN
    assoc, clear = R.counts_reference(ref, case, metric)
    return case, metric, assoc, clear


@pytest.mark.parametrize("n,m", R.COUNT_SHAPES)
def test_line_counts_oracle_and_host_build(n, m):
    case, metric, assoc, clear = counts_setup(n, m)
    s = np.maximum(case["s"], 1e-200)
    with np.errstate(all="ignore"):
        R.check_counts(em.calc_vp_line_counts(case["v"], case["lp"], s, metric, case["lweight"], 1.96 ** 2), case, assoc, clear)
    R.check_counts(simlib.line_counts(case["lp"], case["v"], case["s"], metric, case["lweight"]), case, assoc, clear)
