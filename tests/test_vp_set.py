"""The extended-precision restatements of calc_vp_line_counts, split_best_vp and merge_vps (tests/vp_set_reference.py) held
to the reference's own recorded results (tests/golden/vpset, scripts/make_vpset_goldens.py), and the margin of every
decision of every committed case.  CPU only; reads the golden files, never the reference tree."""
import glob
import os

import numpy as np
import pytest

from conftest import ROOT
import vp_set_reference as R
from em_phase_reference import LD, U, ld

GOLDEN = os.path.join(ROOT, "tests", "golden", "vpset")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))
EXPECTED = 15 + len(R.SPLIT_SPECS) + len(R.MERGE_SPECS)


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def names(prefix):
    return [os.path.basename(f)[:-4] for f in FILES if os.path.basename(f).startswith(prefix)]


def counts_ref(g):
    return R.counts_reference(g["vp"], g["lp"], g["s"], g["metric"], g["lweights"], float(g["thresh"]), g.get("vp_assoc"))


def split_ref(g):
    return R.split_reference(g["v"], g["s"], g["lp"], g["l"], g["w"], g["lw"], g["langle"], float(g["min_diff"]))


def merge_ref(g):
    return R.merge_reference(g["v"], g["s"], g["l"], float(g["thresh"]), g["lw"], g["lsim"], float(g["wbias"]),
                             (R._grid(), g["prior_weights"], float(g["prior_sigma"])), g["lp"], float(g["max_stdd"]))


def angle_between(a, b):
    a, b = ld(a), ld(b)
    c = abs(np.dot(a, b)) / np.sqrt(np.dot(a, a) * np.dot(b, b))
    return float(np.arccos(min(c, LD(1))))


def test_every_case_is_committed():
    assert len(FILES) == EXPECTED
    assert len(names("counts_")) == 15 and set(names("split_")) == set(R.SPLIT_SPECS) and set(names("merge_")) == set(R.MERGE_SPECS)


def test_generators_reproduce_the_committed_inputs():
    """the golden files hold exactly what the seeded generators make: the GPU tests may use either"""
    for name, c in R.counts_cases().items():
        g = load(name)
        for k, v in c.items():
            assert np.array_equal(g[k], v), (name, k)
    for name in R.SPLIT_SPECS:
        g, c = load(name), R.split_case(name)
        for k, v in c.items():
            assert np.array_equal(g[k], v), (name, k)
    for name in R.MERGE_SPECS:
        g = load(name)
        c = R.merge_case(name, int(g["attempt"]))
        for k, v in c.items():
            assert k == "cnn" or np.array_equal(g[k], v), (name, k)


@pytest.mark.parametrize("name", sorted(R.MERGE_SPECS))
def test_merge_cases_end_as_their_spec_says(name):
    assert R.merge_outcome(merge_ref(load(name))) == R.MERGE_SPECS[name][5:]


@pytest.mark.parametrize("name", names("counts_"))
def test_counts_restatement(name):
    g = load(name)
    counts, cw, assoc, mg = counts_ref(g)
    assert mg.clear(), mg.worst()
    assert np.array_equal(counts, g["out_counts"]) and np.array_equal(assoc, g["out_vp_assoc"])
    # the reference's running fp64 sum of at most N positive terms: N roundings of at most u times the final sum
    n = g["lp"].shape[0]
    assert np.all(np.abs(cw - ld(g["out_counts_weighted"])) <= n * U * np.abs(cw))


@pytest.mark.parametrize("name", names("split_"))
def test_split_restatement(name):
    g = load(name)
    r = split_ref(g)
    assert r["margins"].clear(), r["margins"].worst()
    assert r["split"] == int(g["out_split"]) and r["v"].shape == g["out_v"].shape
    want = g["out_labels"]
    got = r["labels"] if r["labels"] is not None else np.full(want.shape, -1)
    assert np.array_equal(got, want), "cluster labels"
    for k in range(r["v"].shape[0]):
        assert angle_between(r["v"][k], g["out_v"][k]) <= R.PARITY_RAD
    assert np.all(np.abs(ld(r["s"]) - ld(g["out_s"])) <= 2 * U * np.abs(ld(g["out_s"])))


@pytest.mark.parametrize("name", names("merge_"))
def test_merge_restatement(name):
    g = load(name)
    r = merge_ref(g)
    assert r["margins"].clear(), r["margins"].worst()
    assert np.array_equal(r["kept"], g["out_kept"]) and r["v"].shape == g["out_v"].shape
    rank1 = any((not q["none"]) and q["sv"][1] <= 1e-6 * q["sv"][0] for q in r["rounds"])
    for k in range(r["v"].shape[0]):
        if not rank1:                                            # one line: LAPACK's choice in a null PLANE, no direction to compare
            assert angle_between(r["v"][k], g["out_v"][k]) <= R.PARITY_RAD
    rel = np.abs(ld(r["s"]) - ld(g["out_s"])) / np.abs(ld(g["out_s"]))
    assert np.all(rel <= R.GOLDEN_S_REL)


def test_golden_variance_bar(capsys):
    """GOLDEN_S_REL bounds the relative deviation of the reference's recorded s from the restatement over ALL committed
    split and merge cases, and is not slack by more than a factor of 20 (so that it stays a measurement)."""
    worst = LD(0)
    for name in names("split_") + names("merge_"):
        g = load(name)
        r = split_ref(g) if name.startswith("split_") else merge_ref(g)
        worst = max(worst, (np.abs(ld(r["s"]) - ld(g["out_s"])) / np.abs(ld(g["out_s"]))).max())
    with capsys.disabled():
        print("\nlargest relative deviation of the recorded s from the restatement: %.3g (bar %.3g)" % (float(worst), R.GOLDEN_S_REL))
    assert worst <= R.GOLDEN_S_REL
    assert worst >= R.GOLDEN_S_REL / 20


def test_no_case_is_left_out_of_the_margin_check():
    checked = 0
    for f in FILES:
        name = os.path.basename(f)[:-4]
        g = load(name)
        mg = counts_ref(g)[3] if name.startswith("counts_") else (split_ref(g) if name.startswith("split_") else merge_ref(g))["margins"]
        assert mg.clear(), (name, mg.worst())
        checked += 1
    assert checked == EXPECTED


# ---- exact ties: the documented rule (first index) ------------------------------------------------------------------------
def tie_counts_case():
    g = load("counts_n65_m2")
    metric = g["metric"].copy()
    metric[1] = metric[0]                                        # two equal metric entries for every line
    return g, metric


def tie_merge_case():
    g = load("merge_m2_above")
    v = np.stack([g["v"][0], g["v"][1], g["v"][0], g["v"][1]])   # VPs 0 == 2 and 1 == 3, bit for bit
    return g, v, np.full(4, 1e-4)


def test_ties_take_the_first_index():
    g, metric = tie_counts_case()
    assoc = R.counts_reference(g["vp"], g["lp"], g["s"], metric, np.ones(65), 1e300)[2]
    assert np.all(assoc == 0)
    g, v, s = tie_merge_case()
    a = R.angle_matrix(v)
    assert a[0, 2] == a[1, 3] == a.min() and int(np.argmin(a.ravel())) == 2      # (0, 2) is the first row-major minimum
    r = R.merge_reference(v, s, g["l"], float(g["thresh"]), g["lw"], g["lsim"], 1.0,
                          (R._grid(), g["prior_weights"], float(g["prior_sigma"])), g["lp"], 0.01)
    assert [(q["j"], q["k"]) for q in r["rounds"]][0] == (0, 2)


def test_calc_angle_to_other_vp_on_the_host():
    from vanishing_points_2017_amd import vp_localisation as V
    v = R._unit(np.random.RandomState(3).normal(size=(3, 5, 3)))
    a = V.calc_angle_to_other_vp(v, 1, 2)
    want = R.angle_matrix(v[1])[2]
    assert a.shape == (5,) and a[2] == np.pi and np.allclose(a, want.astype(np.float64), rtol=0, atol=1e-15)
    assert V.calc_angle_to_other_vp(v[:, :1], 0, 0) == np.pi      # one VP: squeezing leaves a scalar (:693-694)


def test_argument_errors_need_no_gpu():
    from vanishing_points_2017_amd import vp_localisation as V
    lp, v = np.zeros((4, 4)), np.zeros((1, 65, 3))
    with pytest.raises(ValueError, match="dotprod"):
        V.calc_vp_line_counts(v[0, :2], None, lp, np.ones(2), np.ones((2, 4)), np.ones(4), "dotprod")
    with pytest.raises(ValueError, match="area"):
        V.merge_vps(0, v[:, :2], np.ones(2), None, 1e-3, None, None, 1, None, lp, None, "area")
    with pytest.raises(ValueError, match="numClusters"):
        V.split_best_vp(0, v[:, :2], np.ones(2), lp, None, None, None, None, numClusters=3)
    with pytest.raises(ValueError, match="at most 64"):
        V.split_best_vp(0, v, np.ones(65), lp, None, None, None, None)
    with pytest.raises(ValueError, match="at most 64"):
        V.merge_vps(0, v, np.ones(65), None, 1e-3, None, None, 1, None, lp, None, "angle")
    with pytest.raises(ValueError, match="at most 64"):
        V.calc_vp_line_counts(v[0], None, lp, np.ones(65), np.ones((65, 4)), np.ones(4), "angle")


def _batch_inputs():
    """Two images (N = 4 and 3 lines, M = 2 and 1 VPs) as lists: shapes are all these checks read."""
    n, m = (4, 3), (2, 1)
    z = lambda *shape: [np.zeros((k,) + shape) for k in n]
    return {"lps": z(4), "ls": z(3), "lw": z(), "ang": z(), "lsims": [np.zeros((k, k)) for k in n],
            "vs": [np.zeros((k, 3)) for k in m], "ss": [np.ones(k) for k in m], "w": [np.zeros((j, k)) for j, k in zip(m, n)],
            "assoc": [np.zeros(k, np.int64) for k in n]}


def test_counts_batch_errors_need_no_gpu():
    from vanishing_points_2017_amd import vp_localisation as V
    g = _batch_inputs()
    cat = {k: np.concatenate([a.reshape(a.shape[0], -1) if k in ("lps", "vs") else a.ravel() for a in v]) for k, v in g.items()}
    with pytest.raises(ValueError, match="decision_metrics or vp_assocs is needed"):
        V.calc_vp_line_counts_batch(g["vs"], g["lps"], g["ss"], None, g["lw"])
    with pytest.raises(ValueError, match="the decision metrics hold 10 elements, the images' M x N sum to 11"):
        V.calc_vp_line_counts_batch(g["vs"], g["lps"], g["ss"], [g["w"][0], g["w"][1][:, :2]], g["lw"])
    with pytest.raises(ValueError, match="ss holds 2 elements, expected 3"):
        V.calc_vp_line_counts_batch(g["vs"], g["lps"], g["ss"][:1], g["w"], g["lw"])
    with pytest.raises(ValueError, match="lweights holds 8 elements, expected 7"):
        V.calc_vp_line_counts_batch(g["vs"], g["lps"], g["ss"], g["w"], [np.zeros(4), np.zeros(4)])
    with pytest.raises(ValueError, match="vp_assocs holds 6 elements, expected 7"):
        V.calc_vp_line_counts_batch(g["vs"], g["lps"], g["ss"], None, g["lw"], vp_assocs=[g["assoc"][0], g["assoc"][1][:2]])
    with pytest.raises(ValueError, match="lps and vps describe 2 and 1 images"):
        V.calc_vp_line_counts_batch(g["vs"][:1], g["lps"], g["ss"], g["w"], g["lw"])
    # the concatenated form
    off = {"line_offsets": [0, 4, 7], "vp_offsets": [0, 2, 3]}
    with pytest.raises(ValueError, match="the decision metrics hold 10 elements, the images' M x N sum to 11"):
        V.calc_vp_line_counts_batch(cat["vs"], cat["lps"], cat["ss"], cat["w"][:-1], cat["lw"], **off)
    with pytest.raises(ValueError, match="lweights holds 6 elements, expected 7"):
        V.calc_vp_line_counts_batch(cat["vs"], cat["lps"], cat["ss"], cat["w"], cat["lw"][:-1], **off)
    with pytest.raises(ValueError, match="lps offsets must rise from 0 to 7"):
        V.calc_vp_line_counts_batch(cat["vs"], cat["lps"], cat["ss"], cat["w"], cat["lw"], line_offsets=[0, 4, 8], vp_offsets=[0, 2, 3])


def test_split_batch_errors_need_no_gpu():
    from vanishing_points_2017_amd import vp_localisation as V
    g = _batch_inputs()
    with pytest.raises(ValueError, match="the weight matrices do not hold the images' M x N elements"):
        V.split_best_vp_batch(g["vs"], g["ss"], g["lps"], g["ls"], g["w"][:1], g["lw"], g["ang"])
    with pytest.raises(ValueError, match="lines holds 6 rows, expected 7"):
        V.split_best_vp_batch(g["vs"], g["ss"], g["lps"], [g["ls"][0], g["ls"][1][:2]], g["w"], g["lw"], g["ang"])
    with pytest.raises(ValueError, match="ss holds 2 rows, expected 3"):
        V.split_best_vp_batch(g["vs"], g["ss"][:1], g["lps"], g["ls"], g["w"], g["lw"], g["ang"])
    with pytest.raises(ValueError, match="lineWeights holds 4 rows, expected 7"):
        V.split_best_vp_batch(g["vs"], g["ss"], g["lps"], g["ls"], g["w"], g["lw"][:1], g["ang"])
    with pytest.raises(ValueError, match="lineAngles holds 8 rows, expected 7"):
        V.split_best_vp_batch(g["vs"], g["ss"], g["lps"], g["ls"], g["w"], g["lw"], [np.zeros(4), np.zeros(4)])
    with pytest.raises(ValueError, match="linePoints and vs describe 2 and 1 images"):
        V.split_best_vp_batch(g["vs"][:1], g["ss"], g["lps"], g["ls"], g["w"], g["lw"], g["ang"])


def test_merge_batch_errors_need_no_gpu():
    from vanishing_points_2017_amd import probability_functions as P, vp_localisation as V
    g = _batch_inputs()
    par = P.PDFParams(means=None, weights=np.zeros((2, 400), np.float32), sigma=0.1)

    def merge(ls=g["ls"], ss=g["ss"], lw=g["lw"], lsims=g["lsims"], par=par, vs=g["vs"]):
        return V.merge_vps_batch(vs, ss, ls, 1e-3, lw, lsims, 1, par, g["lps"])

    for bad in (g["lsims"][:1], [g["lsims"][0], np.zeros((3, 2))], np.zeros(24)):        # 4 x 4 and 3 x 3: 25 elements
        with pytest.raises(ValueError, match="lsims must hold one N x N matrix per image"):
            merge(lsims=bad)
    with pytest.raises(ValueError, match=r"pdfpar.weights must be \(2, 400\), one row per image"):
        merge(par=par._replace(weights=np.zeros((1, 400), np.float32)))
    with pytest.raises(ValueError, match="ls holds 6 rows, expected 7"):
        merge(ls=[g["ls"][0], g["ls"][1][:2]])
    with pytest.raises(ValueError, match="ss holds 2 rows, expected 3"):
        merge(ss=g["ss"][:1])
    with pytest.raises(ValueError, match="lweights holds 4 rows, expected 7"):
        merge(lw=g["lw"][:1])
    with pytest.raises(ValueError, match="lps and vs describe 2 and 1 images"):
        merge(vs=g["vs"][:1])
    with pytest.raises(ValueError, match="at most 64"):
        merge(vs=[np.zeros((65, 3)), g["vs"][1]])
