"""The scoring's device code (csrc/score_device.hpp) compiled for the host by tests/hostsim/sim_score.cpp and run serially
against NumPy: the horizon error equals calc_horizon.horizon_error byte for byte, the sorted errors equal np.sort, and the
AUC agrees with auc.calc_auc within 2 (n + 4) 2^-53.  The kernels themselves: tests/test_gpu_benchmark_real.py, which
imports the tables below.

The AUC bound is derived, not measured: both sides add the same at most n + 1 non-negative terms -- each the same
expression, so each the same bits -- whose sum is at most `cutoff`; a sum of m such terms in any order is within
(m - 1) 2^-53 of the exact sum relative to it, and the division by the cutoff adds one rounding on each side of a value
that is at most 1.

NumPy's default argsort is an insertion sort, and so stable, only up to 16 elements; beyond that it reorders equal keys
(on sorted input too), and auc.calc_auc, which argsorts the curve's points (auc.py:32), then depends on that order
wherever two points with x <= cutoff share their x.  The device rule is np.argsort(kind="stable") (include/vpk.h).  So
inputs with ties at or below the cutoff are held to auc.calc_auc for n <= 15 and to `stable_calc_auc` -- calc_auc with
the stable kind, checked here to equal calc_auc for n <= 15 -- beyond; ties above the cutoff touch no term and are held to
auc.calc_auc at every n.  One error alone is held to the restatement too: calc_auc squeezes its input (auc.py:7) and has
no vector left to sort."""
import ctypes
import os

import numpy as np
import pytest

from hostsim import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))

V, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
ERROR_DIMS = ((640, 480), (427, 640), (1, 1))
ERROR_KINDS = ("random", "horizontal", "th0_equals_th1", "t2_zero", "t2_zero_nan", "nan_end_points", "inf_end_points")
AUC_N = (1, 2, 15, 63, 64, 65, 257, 2018)
CUTOFF = 0.25


def build_sim():
    lib = hostbuild.load("score")
    lib.sim_horizon_error.argtypes = [I, V, V, V, V]
    lib.sim_auc.argtypes = [I, V, D, V, V]
    return lib


@pytest.fixture(scope="module")
def sim():
    return build_sim()


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def auc_bound(n):
    return 2 * (n + 4) * 2.0 ** -53


# ---- errors ---------------------------------------------------------------------------------------------------------
def error_table(batch, seed=21):
    """(horizon B x 15, true_horizon B x 3, dims B x 2): the kinds of ERROR_KINDS and the sizes of ERROR_DIMS in turn."""
    rs = np.random.RandomState(seed)
    horizon = rs.uniform(-2.0, 2.0, (batch, 15))
    horizon[:, 0], horizon[:, 2], horizon[:, 3], horizon[:, 5] = 1.0, 1.0, -1.0, 1.0
    th = rs.normal(size=(batch, 3))
    dims = np.array([ERROR_DIMS[(b // len(ERROR_KINDS)) % len(ERROR_DIMS)] for b in range(batch)], dtype=np.int32).reshape(batch, 2)
    for b in range(batch):
        kind = ERROR_KINDS[b % len(ERROR_KINDS)]
        if kind == "horizontal":
            th[b, 0] = 0.0 if b % 2 else -0.0
        elif kind == "th0_equals_th1":
            th[b, 0] = th[b, 1]
        elif kind == "t2_zero":                                  # np.cross(th, [+-1, 0, 1])[2] = -+th[1]
            th[b, 1] = 0.0
        elif kind == "t2_zero_nan":                              # ... and [1] = th[2] - th[0] = 0 for the first end point: 0 / 0
            th[b, 1] = 0.0
            th[b, 2] = th[b, 0]
        elif kind == "nan_end_points":
            horizon[b, 1 if b % 2 else 4] = np.nan
        elif kind == "inf_end_points":
            horizon[b, 1], horizon[b, 4] = np.inf, -np.inf if b % 2 else 0.5
    return np.ascontiguousarray(horizon), np.ascontiguousarray(th), dims


def numpy_errors(horizon, th, dims):
    from vanishing_points_2017_amd import calc_horizon as ch
    out = np.empty(horizon.shape[0])
    with np.errstate(all="ignore"):
        for b in range(horizon.shape[0]):
            out[b] = ch.horizon_error(horizon[b, 0:3], horizon[b, 3:6], th[b], (int(dims[b, 1]), int(dims[b, 0])))
    return out


def sim_errors(sim, horizon, th, dims):
    out = np.full(horizon.shape[0], -7.25)
    assert sim.sim_horizon_error(horizon.shape[0], _p(horizon), _p(th), _p(dims), _p(out)) == 0
    return out


@pytest.mark.parametrize("batch", (0, 1, 65, 1025))
def test_errors_equal_numpy_byte_for_byte(sim, batch):
    table = error_table(batch)
    got, want = sim_errors(sim, *table), numpy_errors(*table)
    assert got.tobytes() == want.tobytes()
    if batch >= 65:
        assert np.isnan(got).any() and np.isinf(got).any() and np.isfinite(got).sum() >= batch // 3


def test_errors_refuse_an_empty_side(sim):
    horizon, th, dims = error_table(8)
    dims[3, 1] = 0
    out = np.full(8, -7.25)
    assert sim.sim_horizon_error(8, _p(horizon), _p(th), _p(dims), _p(out)) == -1 and (out == -7.25).all()


# ---- AUC ------------------------------------------------------------------------------------------------------------
def stable_calc_auc(error_array, cutoff=CUTOFF):
    """auc.calc_auc with np.argsort(kind="stable") where it sorts the curve's points: the rule of include/vpk.h."""
    err = np.sort(np.asarray(error_array, dtype=np.float64))
    n = err.shape[0]
    pts = np.zeros((n, 2))
    pts[:, 0] = err
    pts[:, 1] = (np.arange(n) + 1) * 1.0 / n
    mid = 1.
    for i in range(1, n):
        if err[i - 1] < cutoff < err[i]:
            mid = (err[i - 1] * pts[i - 1, 1] + err[i] * pts[i, 1]) / (err[i] + err[i - 1])
    tail = np.array([cutoff, 1]) if pts[-1, 0] < cutoff else np.array([cutoff, mid])
    pts = np.vstack([pts, tail])
    pts = pts[np.argsort(pts[:, 0], kind="stable"), :]
    sel = pts[:, 0] <= cutoff
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    return trapezoid(pts[sel, 1], pts[sel, 0]) / cutoff


def auc_cases(n, seed=22):
    """[(name, errors, reference)]: reference "numpy" = auc.calc_auc, "stable" = stable_calc_auc (the module docstring says
    when).  Errors are shuffled: the kernels must not rely on their order."""
    rs = np.random.RandomState(seed + n)
    lo, hi = max(1, n // 2), n - max(1, n // 2)
    cases = [("all_below", rs.uniform(0.0, 0.2499, n), "numpy"),
             ("all_above", rs.uniform(0.2501, 3.0, n), "numpy"),
             ("one_crossing", np.concatenate([rs.uniform(0.0, 0.2499, lo), rs.uniform(0.2501, 1.0, hi)]), "numpy"),
             ("equal_above", np.concatenate([rs.uniform(0.0, 0.2499, lo), np.full(hi, 0.3)]), "numpy"),
             ("nan_and_inf", np.concatenate([rs.uniform(0.0, 0.5, lo), rs.choice([np.nan, np.inf, 0.7], hi)]), "numpy")]
    ties = "numpy" if n <= 15 else "stable"
    cases.append(("all_equal_below", np.full(n, 0.125), ties))
    cases.append(("three_values", rs.choice([0.0625, 0.125, 0.375], n), ties))
    cases.append(("equal_to_cutoff", np.concatenate([rs.uniform(0.0, 0.2, lo), np.full(hi, CUTOFF)]), ties))
    if n >= 3:       # below, [equal to the cutoff ...], above: no strict crossing although the curve crosses
        third = n // 3
        cases.append(("crossing_through_ties", np.concatenate([rs.uniform(0.0, 0.2, third), np.full(n - 2 * third, CUTOFF),
                                                               rs.uniform(0.3, 1.0, third)]), ties))
        # two separate runs of ties with the strict crossing between them
        cases.append(("ties_either_side", np.concatenate([np.full(third, 0.2), np.full(n - 2 * third, 0.3), np.full(third, 0.1)]), ties))
    if n >= 2:
        cases.append(("all_nan_but_one", np.concatenate([[0.1], np.full(n - 1, np.nan)]), "numpy"))
    cases.append(("all_nan", np.full(n, np.nan), "numpy"))
    return [(name, np.ascontiguousarray(rs.permutation(e)), ref) for name, e, ref in cases]


def reference_auc(err, ref, cutoff=CUTOFF):
    from vanishing_points_2017_amd import auc
    with np.errstate(all="ignore"):
        if ref == "numpy" and err.shape[0] > 1:      # calc_auc squeezes its input (auc.py:7): one error is no vector to it
            return auc.calc_auc(err.copy(), cutoff=cutoff)[0]
        return stable_calc_auc(err, cutoff)


def sim_auc(sim, err, cutoff=CUTOFF):
    n = err.shape[0]
    srt, out = np.full(max(n, 1), -7.25), np.full(1, -7.25)
    rc = sim.sim_auc(n, _p(err), cutoff, _p(srt), _p(out))
    return rc, srt[:n], out[0]


@pytest.mark.parametrize("n", AUC_N)
def test_auc_equals_calc_auc_within_the_derived_bound(sim, n):
    for name, err, ref in auc_cases(n):
        rc, srt, got = sim_auc(sim, err)
        assert rc == 0, name
        assert np.array_equal(srt, np.sort(err), equal_nan=True), name
        want = reference_auc(err, ref)
        if np.isnan(want):                   # a crossing from a number to inf: mid = inf / inf, on both sides
            assert np.isnan(got) and name == "nan_and_inf", (name, n, got)
            continue
        assert abs(got - want) <= auc_bound(n), (name, n, got, want)
        assert 0.0 <= got <= 1.0 + auc_bound(n), name


@pytest.mark.parametrize("n", (2, 3, 15))
def test_the_stable_restatement_is_calc_auc_where_numpy_is_stable(n):
    for name, err, _ in auc_cases(n):
        with np.errstate(all="ignore"):
            assert np.array_equal(stable_calc_auc(err), reference_auc(err, "numpy"), equal_nan=True), name


def test_auc_in_words(sim):
    """Values worked by hand: one error below the cutoff; an error equal to the cutoff comes before the tail point; NaN
    counts in the fractions."""
    assert sim_auc(sim, np.array([0.125]))[2] == (0.25 - 0.125) * (1.0 + 1.0) / 2.0 / 0.25
    # points (0.125, 1/2), (0.25, 1), tail (0.25, mid = 1): the tail adds a zero-width term
    assert sim_auc(sim, np.array([0.25, 0.125]))[2] == (0.125 * 1.5 / 2.0 + 0.0) / 0.25
    # (0.125, 1/2), (nan, 1): largest error not below the cutoff, no strict crossing -> mid = 1
    assert sim_auc(sim, np.array([np.nan, 0.125]))[2] == (0.125 * 1.5 / 2.0) / 0.25
    assert sim_auc(sim, np.array([0.5, np.inf]))[2] == 0.0
    # the crossing: mid = (0.125 * 0.5 + 0.5 * 1) / 0.625
    mid = (0.125 * 0.5 + 0.5 * 1.0) / (0.5 + 0.125)
    assert sim_auc(sim, np.array([0.5, 0.125]))[2] == (0.125 * (mid + 0.5) / 2.0) / 0.25


def test_auc_limits(sim):
    assert sim_auc(sim, np.zeros(0))[0] == -1
    err = np.zeros(65537)
    srt, out = np.full(4, -7.25), np.full(1, -7.25)
    assert sim.sim_auc(65537, _p(err), CUTOFF, _p(srt), _p(out)) == -5 and (srt == -7.25).all() and out[0] == -7.25


def test_entry_points_are_declared_and_exported():
    from vanishing_points_2017_amd import _lib, auc, calc_horizon
    assert {"vpk_horizon_error_batch", "vpk_auc"} <= set(_lib.EXPORTS)
    assert callable(calc_horizon.horizon_error_batch_device) and callable(auc.calc_auc_device)
    text = open(os.path.join(HERE, "..", "include", "vpk.h")).read()
    assert "int vpk_horizon_error_batch(" in text and "int vpk_auc(" in text
    from vanishing_points_2017_amd import build
    assert build.UNITS["vpk_score.hip"] == ["-ffp-contract=off"]
