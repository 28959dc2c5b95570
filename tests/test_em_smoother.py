"""CPU twins of tests/test_gpu_em_smoother.py (cases, references and bars: tests/em_smoother_reference.py):

  * the float64 NumPy expression of weight_matrix meets every bar on every generated case -- the condition that no bar is
    tighter than float64 arithmetic allows, none being fitted to a kernel;
  * the host build of the UNMODIFIED device source meets them through simlib.weight_matrix (the smoother stages its
    panel) and simlib.estep_smooth (the E-step hands it over), under LDS budgets that make the one-lane build take
    smooth_blocks, smooth_full in passes and the plan-1 hand-off, with bit-identical results either way;
  * the restated dispatch (path_of) gives the issue's kernel for every row of the path table.

The one-lane build never takes the row-sliced or the sparse kernel (they need a 64-lane wave).
"""
import functools

import numpy as np
import pytest

import em_smoother_reference as S
from hostsim import simlib

HOST_BUDGETS = (64, 96, 700, 2048, 6144)


def _bias(n, m):
    return S.BIASES[(n + m) % 3]


@functools.lru_cache(maxsize=None)
def staged_setup(kind, n, m, bias):
    case = {"sparse": S.sparse_case, "coded": S.coded_case, "edge": S.edge_slice_case}[kind](n, m)
    w, bar = S.smooth_reference(case["p_vl"] * case["lweight"][None, :], 0 * case["p_vl"], case["lweight"], case["lsim"], bias)
    return case, w, (bar if kind == "sparse" else S.coded_bar(w))


# ---- the reference module's own tools ------------------------------------------------------------------------------
def test_generators_give_what_they_promise():
    c = S.sparse_case(257, 64)
    assert 0.80 < (c["p_vl"] == 0).mean() < 0.87 and not c["p_vl"][32].any() and not c["p_vl"][:, -1].any()
    nz = c["p_vl"][c["p_vl"] > 0]
    assert nz.min() < 1e-290 and nz.max() > 0.1 and (c["p_vl"] >= 0).all()
    assert 0.05 < (c["lweight"] == 0).mean() < 0.16 and c["lweight"].max() < 0.4 and (c["lweight"] != 1).all()
    ls = c["lsim"]
    assert 0.27 < (ls == 0).mean() < 0.33 and not np.diag(ls).any() and (ls != ls.T).mean() > 0.8
    assert ls[ls > 0].min() < 1e-11 and ls.max() > 0.9
    c = S.coded_case(129, 40)
    assert (c["lsim"] != c["lsim"].T).mean() > 0.9 and (np.log2(c["lweight"]) % 1 == 0).all()
    w_ = c["p_vl"] * c["lweight"][None, :]
    for order in (np.arange(129), np.arange(129)[::-1], np.random.RandomState(0).permutation(129)):
        acc = np.zeros((40, 129))
        for j in order:                                      # exact in every order
            acc += w_[:, j:j + 1] * c["lsim"][j:j + 1, :]
        assert np.array_equal(acc, (S.ld(w_) @ S.ld(c["lsim"])).astype(np.float64))
    e = S.edge_slice_case(9, 8)
    assert np.flatnonzero(e["p_vl"][0]).tolist() == [8] and np.flatnonzero(e["p_vl"][1]).tolist() == [2]
    assert S.rs_jchunk(9) == 2                               # slices of two rows: slice 4 has one line, 5 .. 7 none


def test_coded_case_sees_a_misplaced_operand():
    """What the coded values are for: a transposed lsim, a dropped row, a duplicated row or two swapped VPs move the exact
    result by far more than the bar."""
    n, m = 65, 33
    case, w, bar = staged_setup("coded", n, m, 1.0)
    p, lw, ls = case["p_vl"], case["lweight"], case["lsim"]
    wrong = [S.numpy_expression(p, lw, ls.T.copy(), 1.0)]
    q = p.copy(); q[:, 64] = 0; wrong.append(S.numpy_expression(q, lw, ls, 1.0))
    q = p.copy(); q[:, 9] = p[:, 8] * lw[8] / lw[9]; wrong.append(S.numpy_expression(q, lw, ls, 1.0))
    q = p.copy(); q[[32, 0]] = p[[0, 32]]; wrong.append(S.numpy_expression(q, lw, ls, 1.0))
    for bad in wrong:
        assert (np.abs(S.ld(bad) - w) > 1e6 * bar).any()


def test_path_table_restated():
    """smooth_plan / smooth_dispatch restated (path_of) send every row of the issue's table to the kernel it names."""
    D = S.DEFAULT_BUDGET

    def k(n, m, wt, mode, estep=False):
        info = S.expected_info(n, m, wt, mode, estep=estep)
        return S.path_of(n, m, wt, mode, info)

    for n, m in S.ROWS_SHAPES:
        assert k(n, m, D, 0).kernels == ("rows<%d>" % ((m + 7) // 8),)
        assert k(n, m, D, 0, estep=True).handed and not k(n, m, D, 0).handed
    assert {k(n, m, D, 0).kernels[0] for n, m in S.ROWS_SHAPES} == {"rows<1>", "rows<2>", "rows<3>", "rows<4>"}
    assert [k(n, m, D, 0).kernels for n, m in S.SECOND_PASS_SHAPES] == [("rows<4>", "rows<1>"), ("rows<4>", "rows<1>"), ("rows<4>", "rows<4>")]
    assert [k(n, m, D, 2).kernels[0] for n, m in S.SPARSE_SHAPES] == ["sparse<%d>" % c for c in (1, 2, 3, 4, 5, 6, 7, 7)] + ["rows<3>"]
    assert [k(n, m, D, 0).kernels[0] for n, m in S.FULL_EDGE_SHAPES] == ["rows<1>", "full<1,2>:direct", "full<2,2>:direct", "rows<1>"]
    assert [k(n, m, D, 1).kernels[0] for n, m in S.FULL_EDGE_SHAPES] == ["full<1,2>:sliced", "full<1,2>:direct", "full<2,2>:direct", "full<1,2>:sliced"]
    assert [k(n, m, D, 1).kernels[0] for n, m in S.FULL_C_SHAPES] == ["full<%d,%d>:sliced" % (nt, c) for c in (1, 2) for nt in (1, 2, 3, 4)]
    assert k(65, 33, 6144, 0).kernels == ("rows<2>", "rows<2>", "rows<1>") and k(129, 40, 6144, 0).kernels == ("rows<1>",) * 5
    assert k(129, 40, 2048, 0).kernels == ("full<1,2>:sliced",) * 5
    assert k(128, 24, 2048, 0).kernels == ("full<2,2>:sliced", "full<1,2>:sliced")
    assert k(65, 33, 2048, 0).kernels == ("full<3,2>:sliced", "full<2,2>:sliced")
    assert k(16, 9, 96, 0).kernels == ("blocks<1>",) and k(129, 40, 96, 0).kernels == ("blocks<2>",) and k(9, 8, 64, 0).kernels == ("blocks<1>",)
    assert k(513, 32, D, 0, estep=True).kernels == ("full<4,2>:sliced",) and k(513, 32, D, 0, estep=True).handed


# ---- the float64 NumPy expression meets every bar ---------------------------------------------------------------
@pytest.mark.parametrize("n,m", S.CPU_SHAPES)
def test_numpy_expression_meets_the_bound(n, m):
    """sparse_case under the three biases: float64 NumPy stays inside the first-order bound (printed: 0.14 of it at the
    worst on these shapes)."""
    for bias in S.BIASES:
        case, w, bar = staged_setup("sparse", n, m, bias)
        got = S.numpy_expression(case["p_vl"], case["lweight"], case["lsim"], bias)
        r = S.check_smooth(got, w, bar, "numpy sparse")
        print("N=%d M=%d bias=%g float64 NumPy error / bound %.3g" % (n, m, bias, r))


@pytest.mark.parametrize("n,m", [(9, 8), (17, 17), (65, 33), (129, 40), (257, 64), (1025, 8)])
def test_numpy_expression_meets_the_coded_bar(n, m):
    for kind in ("coded", "edge"):
        for bias in S.BIASES:
            case, w, bar = staged_setup(kind, n, m, bias)
            S.check_smooth(S.numpy_expression(case["p_vl"], case["lweight"], case["lsim"], bias), w, bar, "numpy " + kind)


@pytest.mark.parametrize("kind", S.NONFINITE)
@pytest.mark.parametrize("n,m", [(9, 8), (64, 32), (65, 33), (129, 40)])
def test_numpy_expression_on_nonfinite_lsim(n, m, kind):
    """Exactly column k is NaN in float64 NumPy (the expected pattern of the GPU test), every other element within the bound."""
    case = S.nonfinite_case(n, m, kind)
    for bias in S.BIASES:
        got = S.numpy_expression(case["p_vl"], case["lweight"], case["lsim"], bias)
        want = np.zeros((m, n), bool)
        want[:, case["k"]] = True
        assert np.array_equal(np.isnan(got), want)
        w, bar = S.smooth_reference(case["p_vl"] * case["lweight"][None, :], 0 * case["p_vl"], case["lweight"], case["lsim"], bias)
        w[:, case["k"]] = np.nan                             # (the extended reference does not overflow where fp64 does)
        S.check_smooth(got, w, bar, "numpy nonfinite")


# ---- the host build ------------------------------------------------------------------------------------------------
def _host_path(n, m, budget, info):
    return S.path_of(n, m, budget, 1, info)                  # one wave of one lane: never the row-sliced kernel, as setting 1


HOST_STAGED = [(9, 8), (16, 9), (17, 17), (65, 33), (128, 24), (129, 40)]


@pytest.mark.parametrize("budget", HOST_BUDGETS)
@pytest.mark.parametrize("n,m", HOST_STAGED)
def test_host_build_staged(n, m, budget):
    path = _host_path(n, m, budget, S.expected_info(n, m, budget, 1, estep=False))
    for kind in ("sparse", "coded", "edge"):
        bias = 1.0 if kind != "sparse" else _bias(n, m)
        case, w, bar = staged_setup(kind, n, m, bias)
        got = simlib.weight_matrix(case["p_vl"], case["lweight"], case["lsim"], bias, lds_doubles=budget)
        S.check_smooth(got, w, bar, "host %s %s" % (kind, path.kernels[0].split(":")[0]))


@pytest.mark.parametrize("kind", S.NONFINITE)
def test_host_build_nonfinite(kind):
    n, m = 65, 33
    case = S.nonfinite_case(n, m, kind)
    for budget in (96, 2048):
        got = simlib.weight_matrix(case["p_vl"], case["lweight"], case["lsim"], 1.0, lds_doubles=budget)
        w, bar = S.smooth_reference(case["p_vl"] * case["lweight"][None, :], 0 * case["p_vl"], case["lweight"], case["lsim"], 1.0)
        w[:, case["k"]] = np.nan
        S.check_smooth(got, w, bar, "host nonfinite")


@functools.lru_cache(maxsize=None)
def handoff_setup(n, m, degenerate=False):
    case = S.handoff_case(n, m, degenerate)
    return (case,) + S.handoff_reference(case)


HOST_HANDOFF = [(1, 1), (3, 3), (64, 5), (65, 8), (129, 9), (129, 32), (65, 33), (129, 64)]


@pytest.mark.parametrize("budget", HOST_BUDGETS)
@pytest.mark.parametrize("n,m", HOST_HANDOFF)
def test_host_build_handoff(n, m, budget):
    """estep() then smooth() in the host build: w bit-identical to the staged smoother on the hook's own p_vl (the panel the
    E-step writes against the panel the smoother stages) and within the bound of the extended reference."""
    case, est, w, bar = handoff_setup(n, m)
    assert np.isfinite(est["p_vl"].astype(np.float64)).all()
    pvl, got, s, info = simlib.estep_smooth(case["lp"], case["cnn"], case["v"], case["s"], case["lweight"], case["lsim"],
                                            case["bias"], lds_doubles=budget)
    assert list(info) == S.expected_info(n, m, budget, 1)
    path = _host_path(n, m, budget, info)
    assert np.array_equal(s, np.maximum(case["s"], 1e-200))
    stag = simlib.weight_matrix(pvl, case["lweight"], case["lsim"], case["bias"], lds_doubles=budget)
    assert np.array_equal(got, stag), "hand-off and staged panel give different bits (%r)" % path
    assert S._ratio(np.abs(S.ld(pvl) - est["p_vl"]), est["b_pvl"]) <= 1.0
    S.check_smooth(got, w, bar, "host hand-off %s" % path.kernels[0].split(":")[0])


def test_host_build_handoff_degenerate_lines():
    """estep_case's zero-length segment and its line through a VP: p_vl is NaN for them and every w with it, either way."""
    case, est, w, bar = handoff_setup(64, 5, True)
    pvl, got, s, info = simlib.estep_smooth(case["lp"], case["cnn"], case["v"], case["s"], case["lweight"], case["lsim"], case["bias"])
    assert info[1] != 0 and np.isnan(got).all() and np.isnan(w.astype(np.float64)).all()
    assert np.isnan(simlib.weight_matrix(pvl, case["lweight"], case["lsim"], case["bias"])).all()


def test_host_build_paths_covered():
    """The budgets above make the one-lane build take smooth_blocks, smooth_full in several passes and the plan-1 hand-off."""
    seen = set()
    for n, m in HOST_HANDOFF:
        for budget in HOST_BUDGETS:
            path = _host_path(n, m, budget, S.expected_info(n, m, budget, 1))
            seen.add((path.kernels[0].split("<")[0], path.handed, len(path.kernels) > 1))
    assert {("blocks", False, False), ("full", False, True), ("full", True, False)} <= seen
