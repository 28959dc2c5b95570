"""calc_vp_line_counts and merge_vps under "dotprod" and "area": the extended-precision restatements of
tests/vp_set_measure_reference.py held to the reference's own recorded results (tests/golden/vpset_measures,
scripts/make_vpset_measure_goldens.py), the margin of every decision of every committed case, the argument errors of the
batch forms, and the host build of csrc/vpset_device.hpp (tests/hostsim/sim_vpset.cpp) held to the GPU tests' bars.
CPU only; reads the golden files, never the reference tree."""
import os

import numpy as np
import pytest

import vp_set_reference as R
import vp_set_measure_reference as RM
from em_phase_reference import LD, U, ld
from vp_set_measure_reference import COUNTS, angle_between, check_counts, check_merge, counts_ref

CASES = [(measure, name) for measure in RM.MEASURES for name in COUNTS + sorted(R.MERGE_SPECS)]
ALL = ("angle",) + RM.MEASURES


def test_every_case_is_committed():
    files = sorted(f for f in os.listdir(RM.GOLDEN) if f.endswith(".npz"))
    assert files == sorted("%s_%s.npz" % c for c in CASES)
    for measure in RM.MEASURES:
        assert RM.golden_names(measure, "counts_") == sorted(COUNTS)
        assert RM.golden_names(measure, "merge_") == sorted(R.MERGE_SPECS) == sorted(RM.MERGE_OUTCOMES[measure])


@pytest.mark.parametrize("measure", RM.MEASURES)
def test_generators_reproduce_the_committed_inputs(measure):
    for name, c in RM.counts_cases(measure).items():
        g = RM.golden(measure, name)
        for k, v in c.items():
            assert np.array_equal(g[k], v), (name, k)
    for name in R.MERGE_SPECS:
        g = RM.golden(measure, name)
        c = RM.merge_case(measure, name, int(g["attempt"]))
        for k, v in c.items():
            assert k == "cnn" or np.array_equal(g[k], v), (name, k)


@pytest.mark.parametrize("measure,name", [(m, n) for m in RM.MEASURES for n in COUNTS])
def test_counts_restatement(measure, name):
    g = RM.golden(measure, name)
    counts, cw, assoc, mg, inside = counts_ref(measure, g)
    assert mg.clear() and mg.worst()[1] > 1e-9, mg.worst()
    assert np.array_equal(counts, g["out_counts"]) and np.array_equal(assoc, g["out_vp_assoc"])
    n = g["lp"].shape[0]
    assert np.all(np.abs(cw - ld(g["out_counts_weighted"])) <= n * U * np.abs(cw))
    if n >= RM.INSIDE_FROM_N:                                    # both branches of :504
        assert RM.INSIDE_MIN <= RM.inside_fraction(inside) <= RM.INSIDE_MAX, RM.inside_fraction(inside)


def test_counts_cases_are_what_they_say():
    for measure in RM.MEASURES:
        q = 0
        for name in COUNTS:
            g = RM.golden(measure, name)
            assert float(g["thresh"]) == (2.57 if q % 2 == 0 else 1.96 ** 2)
            assert ("vp_assoc" in g) == (q % 2 == 1) and (q % 2 == 0 or (g["vp_assoc"] == -1).any())
            assert not g["lweights"][::5].any() and (g["lweights"] == 0).sum() == len(g["lweights"][::5])
            if g["vp"].shape[0] == 2:
                assert g["vp"][1, 2] == 0
            q += 1
    # the reference's counts at the shapes the variances were chosen on
    assert [int(RM.golden("area", n)["out_counts"].sum()) for n in ("counts_n64_m1", "counts_n65_m2", "counts_n513_m64")] == [24, 33, 192]
    assert int(RM.golden("dotprod", "counts_n65_m2")["out_counts"].sum()) == 15


@pytest.mark.parametrize("measure,name", [(m, n) for m in RM.MEASURES for n in sorted(R.MERGE_SPECS)])
def test_merge_restatement(measure, name):
    g = RM.golden(measure, name)
    r = RM.merge_reference_of(measure, g)
    assert r["margins"].clear() and r["margins"].worst()[1] > 1e-9, r["margins"].worst()
    assert float(g["max_stdd"]) == RM.MERGE_OUTCOMES[measure][name][0]
    assert R.merge_outcome(r) == RM.MERGE_OUTCOMES[measure][name][1:]
    assert np.array_equal(r["kept"], g["out_kept"]) and r["v"].shape == g["out_v"].shape
    rank1 = any((not q["none"]) and q["sv"][1] <= 1e-6 * q["sv"][0] for q in r["rounds"])
    for k in range(r["v"].shape[0]):
        if not rank1:                                            # one line: LAPACK's choice in a null PLANE, no direction to compare
            assert angle_between(r["v"][k], g["out_v"][k]) <= R.PARITY_RAD
    rel = np.abs(ld(r["s"]) - ld(g["out_s"])) / np.abs(ld(g["out_s"]))
    assert np.all(rel <= RM.GOLDEN_S_REL[measure])
    if R.merge_outcome(r)[1] == "max_stdd":
        assert (g["out_s"] != g["s"]).sum() == 1, "a merge given up returns the changed s[k] (:666-668)"


@pytest.mark.parametrize("measure", RM.MEASURES)
def test_golden_variance_bar(measure, capsys):
    """GOLDEN_S_REL[measure] bounds the relative deviation of the reference's recorded s from the restatement over ALL
    committed merge cases of the measure, and is not slack by more than a factor of 20 (so that it stays a measurement)."""
    worst = LD(0)
    for name in sorted(R.MERGE_SPECS):
        g = RM.golden(measure, name)
        r = RM.merge_reference_of(measure, g)
        worst = max(worst, (np.abs(ld(r["s"]) - ld(g["out_s"])) / np.abs(ld(g["out_s"]))).max())
    with capsys.disabled():
        print("\n%s: largest relative deviation of the recorded s from the restatement: %.3g (bar %.3g)"
              % (measure, float(worst), RM.GOLDEN_S_REL[measure]))
    assert worst <= RM.GOLDEN_S_REL[measure]
    assert worst >= RM.GOLDEN_S_REL[measure] / 20


# ---- the batch forms' new argument errors need no GPU ---------------------------------------------------------------------
def test_measure_errors_need_no_gpu():
    from vanishing_points_2017_amd import vp_localisation as V
    from vanishing_points_2017_amd.probability_functions import PDFParams
    n, m = (4, 3), (2, 1)
    lps, ls, lw = [np.zeros((k, 4)) for k in n], [np.zeros((k, 3)) for k in n], [np.zeros(k) for k in n]
    vs, ss, w = [np.zeros((k, 3)) for k in m], [np.ones(k) for k in m], [np.zeros((j, k)) for j, k in zip(m, n)]
    with pytest.raises(ValueError, match="pass ls"):
        V.calc_vp_line_counts_batch(vs, lps, ss, w, lw, distance_measure="dotprod")
    with pytest.raises(ValueError, match="ls holds 6 rows, expected 7"):
        V.calc_vp_line_counts_batch(vs, lps, ss, w, lw, distance_measure="dotprod", ls=[ls[0], ls[1][:2]])
    for bad in ("cosine", None, 1):
        with pytest.raises(ValueError, match="distance_measure"):
            V.calc_vp_line_counts_batch(vs, lps, ss, w, lw, distance_measure=bad, ls=ls)
        with pytest.raises(ValueError, match="distance_measure"):
            V.merge_vps_batch(vs, ss, ls, 1e-3, lw, [np.zeros((k, k)) for k in n], 1,
                              PDFParams(means=None, weights=np.zeros((2, 400), np.float32), sigma=0.1), lps, distance_measure=bad)
    # a known measure passes the new checks and reaches the old ones
    for measure in ALL:
        with pytest.raises(ValueError, match="decision_metrics or vp_assocs is needed"):
            V.calc_vp_line_counts_batch(vs, lps, ss, None, lw, distance_measure=measure, ls=ls)
        with pytest.raises(ValueError, match="pdfpar.weights"):
            V.merge_vps_batch(vs, ss, ls, 1e-3, lw, [np.zeros((k, k)) for k in n], 1,
                              PDFParams(means=None, weights=np.zeros((1, 400), np.float32), sigma=0.1), lps, distance_measure=measure)


# ---- CPU twins: the host build of vpset_device.hpp, with the GPU tests' bars ------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    from hostsim import simlib_vpset
    simlib_vpset.lib()
    return simlib_vpset


@pytest.mark.parametrize("measure,name", [(m, n) for m in RM.MEASURES for n in COUNTS])
def test_host_twin_counts(sim, measure, name):
    g = RM.golden(measure, name)
    given = g["vp_assoc"].copy() if "vp_assoc" in g else None
    got = sim.counts(measure, g["vp"], g["lp"], g["l"] if measure == "dotprod" else None, g["s"], g["metric"], g["lweights"],
                     float(g["thresh"]), given)
    check_counts(got, measure, g)
    if given is not None:
        assert np.array_equal(given, g["vp_assoc"]), "the caller's vp_assoc is not written"


@pytest.mark.parametrize("measure,name", [(m, n) for m in RM.MEASURES for n in sorted(R.MERGE_SPECS)])
def test_host_twin_merge(sim, measure, name):
    g = RM.golden(measure, name)
    got = sim.merge(measure, g["v"], g["s"], g["l"], float(g["thresh"]), g["lw"], g["lsim"], float(g["wbias"]), g["prior_weights"],
                    float(g["prior_sigma"]), g["lp"], float(g["max_stdd"]))
    check_merge(got, measure, g, RM.merge_reference_of(measure, g))


def test_host_twin_angle_is_the_committed_angle(sim):
    """the measure parameter leaves "angle" where it was: the existing goldens through the templated functions"""
    import glob
    for f in sorted(glob.glob(os.path.join(os.path.dirname(RM.GOLDEN), "vpset", "counts_n6*.npz"))):
        with np.load(f) as z:
            g = {k: z[k] for k in z.files}
        counts, _, assoc = sim.counts("angle", g["vp"], g["lp"], None, g["s"], g["metric"], g["lweights"], float(g["thresh"]),
                                      g.get("vp_assoc"))
        assert np.array_equal(counts, g["out_counts"]) and np.array_equal(assoc, g["out_vp_assoc"])
