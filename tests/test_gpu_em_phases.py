"""The EM's phase kernels (csrc/em_device.hpp, launched one at a time through the fine-grained entry points of
csrc/vpk_em.hip) held to extended-precision references at their edges.  One workgroup per call.

Inputs, references and bars are those of tests/em_phase_reference.py; tests/test_em_phases.py runs the same inputs through
the host build of the device source and shows that the float64 oracle meets every bar.  Which case enters which path:

  E-step   T = 8 / 4 / 2 lanes per line: N <= 64 / <= 128 / <= 256 with M <= 32 (an LDS panel); T = 1: N = 257, 513
           M < T (empty VP runs): N <= 64 with M = 1, 2, 3, 5; the four-deep unroll tails: every M with M % 4 != 0
           M > 32 (no panel, products parked in pvl, a second round of 32 VPs in the prior loop): M = 33, 40, 64
           the p_l floor, the s floor (1e-300 -> 1e-200), exp_underflow, five sigmas mixed in one call: estep_case
  M-step   soft and hard mode, lapack_null_1row (a = 0, a = -0.0), the hard mode's `continue`, the refinement passes of
           group_null_vector (bundles with s2 / s1 = 1e-2, 1e-4, 1e-6), mstep_lb<8> (N = 512, 513), a second round of VP
           groups (M = 33, 64), idle lanes of a 16-lane group (N = 1, 2, 3, 15), both variance clamps, a NaN variance,
           err > 1.5: mstep_case
  pairwise the tiled pass (N >= 512) and the row-pair pass with odd N and its middle row (N = 3, 5, 11, 65, ...), fewer
           lines than KNN1 / KNN2 (N = 1 .. 10), 128-pair trip tails (N = 129, 130, 257): against NumPy and the reference
  init     the strided npix > 640 branch (a 520-pixel sphere), all-zero slices, fewer maxima than num_max, the border
  counts   lweight == 0, a NaN column (the NaN rule of assign_lines), lines on either side of the outlier threshold
"""
import functools

import numpy as np
import pytest

import em_phase_reference as R
from oracle import em_numpy as em

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def estep_setup(n, m):
    case = R.estep_case(n, m)
    par = em.pdf_params(case["cnn"].copy())
    ref = R.estep_reference(par, case["v"], case["lp"], case["s"])
    with np.errstate(all="ignore"):
        orc = em.calc_probabilities(par, case["v"], case["lp"], case["s"].copy())
    return case, ref, orc


def _estep(case):
    from vanishing_points_2017_amd import kernels
    pv, lvsq, pvl, pl, s = kernels.estep(case["lp"], case["cnn"], case["v"], case["s"])
    return {"p_v": pv, "lvsq": lvsq, "p_vl": pvl, "p_l": pl, "s": s}


def _with_smoother(mode, fn):
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    rt.handle.em_set_smoother(mode)
    try:
        return fn()
    finally:
        rt.handle.em_set_smoother(0)


@pytest.mark.parametrize("n,m", R.estep_shapes())
def test_estep(n, m):
    """p_v, lvsq, p_vl, p_l within their first-order bounds of the extended reference (and the project's flat bars on
    well-conditioned elements), s floored in place, the NaN / Inf pattern exactly the float64 oracle's -- and the same
    bits with one lane per line (vpk_em_set_smoother(1): T = 1 everywhere)."""
    case, ref, orc = estep_setup(n, m)
    out = _estep(case)
    print("estep N=%d M=%d worst error / bar %.3g" % (n, m, R.check_estep(out, case, ref, orc)))
    one = _with_smoother(1, lambda: _estep(case))
    for k in out:
        assert np.array_equal(out[k], one[k], equal_nan=True), "%s: other bits with one lane per line" % k


@functools.lru_cache(maxsize=None)
def mstep_setup(n, m, hard):
    case = R.mstep_case(n, m, hard)
    ref = R.mstep_reference(case["l"], case["w"], case["lvsq"], case["p_vl"], None, case["assoc"], R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH)
    cur = R.mstep_cur(case, ref, lambda k: k % 12)
    return case, ref, cur


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("n,m", R.mstep_shapes())
def test_mstep(n, m, hard):
    """vpk_mstep_full: the null vector within c(N) u s1 / (s2 - s3) of the extended reference (the normal-equations term
    where pass 0 may leave without refinement), its residual within s3 + c(N) u s1 whatever the conditioning, one-row VPs
    as LAPACK's reflector gives them, the variance with both clamps, err and every removal."""
    from vanishing_points_2017_amd import kernels
    case, ref, cur = mstep_setup(n, m, hard)
    out = kernels.mstep_full(case["l"], case["w"], case["lvsq"], case["p_vl"], cur, case["assoc"], R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH)
    print("mstep N=%d M=%d %s worst error / bar %.3g" % (n, m, "hard" if hard else "soft", R.check_mstep(out, case, ref, cur, hard)))
    if n >= 512:       # mstep_lb<8> against mstep_lb<4>: the same lines in the same order per lane, the same bits
        four = _with_smoother(1, lambda: kernels.mstep_full(case["l"], case["w"], case["lvsq"], case["p_vl"], cur, case["assoc"],
                                                             R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH))
        for a, b in zip(out, four):
            assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("n", R.PAIR_N)
def test_pairwise(n):
    """lsim, the kNN score and the angles against oracle.em_numpy (calc_lsim, line_rating_knn with k2 = 4, lines_angles) and
    against the extended reference; the score on the rows whose neighbour and cosine selections are no ties."""
    from vanishing_points_2017_amd import kernels
    lp = R.pairwise_case(n)
    ref = R.pairwise_reference(lp)
    with np.errstate(all="ignore"):
        dist = em.pair_distance_closest(lp)
        orc = (em.calc_lsim(lp, sigma=1, dist=dist), em.line_rating_knn(lp, k2=4, dist=dist), em.lines_angles(lp))
    print("pairwise N=%d worst error / bar %.3g" % (n, R.check_pairwise(kernels.pairwise(lp), lp, ref, orc)))


@pytest.mark.parametrize("ssize,num_max,kind", R.INIT_CASES)
def test_init_vps(ssize, num_max, kind):
    """vpk_init_vps against find_initial_vps and pdf_params: VP count and order exact, VPs to 1e-13, prior weights bit for
    bit.  The response values are distinct float32 numbers by construction: the order among exactly tied responses is a
    property of NumPy's sort, not of this library, and is not tested."""
    from vanishing_points_2017_amd import kernels
    cnn, sphere = R.init_case(ssize, num_max, kind)
    v0, w = kernels.init_vps(cnn, sphere, num_max)
    try:
        want = em.find_initial_vps(sphere, cnn, num_max)
    except ValueError:                                        # np.vstack([]): no cell survives
        want = np.zeros((0, 3))
    assert v0.shape == want.shape
    if want.size:
        assert np.abs(v0 - want).max() <= 1e-13
    assert np.array_equal(w, em.pdf_params(cnn.copy()).weights)


@pytest.mark.parametrize("n,m", R.COUNT_SHAPES)
def test_line_counts(n, m):
    """vpk_line_counts on a real E-step's p_vl (five sigmas in one call) with zero line weights and a NaN column: assignments
    and counts exact on every line whose argmax and threshold margins exceed 1e-9 relative in the extended reference."""
    from vanishing_points_2017_amd import kernels
    case = R.counts_case(n, m)
    par = em.pdf_params(case["cnn"].copy())
    ref = R.estep_reference(par, case["v"], case["lp"], case["s"])
    with np.errstate(all="ignore"):
        orc = em.calc_probabilities(par, case["v"], case["lp"], case["s"].copy())
    metric = np.asarray(orc.vl).copy()
    if m > 1 and n > 3:
        metric[:, 0] = np.nan
    assoc, clear = R.counts_reference(ref, case, metric)
    R.check_counts(kernels.line_counts(case["lp"], case["v"], case["s"], metric, case["lweight"]), case, assoc, clear)


def test_report_worst_ratios():
    """Prints the worst error / bar per phase seen by the tests above (DESIGN.md quotes them)."""
    for k in sorted(R.WORST):
        print("worst error / bar, %-20s %.3g" % (k, R.WORST[k]))
