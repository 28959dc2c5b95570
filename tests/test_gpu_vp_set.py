"""calc_vp_line_counts, split_best_vp and merge_vps on the GPU (vpk_vp_line_counts_batch, vpk_vp_split_batch,
vpk_vp_merge_batch) held to the reference's recorded results (tests/golden/vpset) and to the extended-precision
restatements of tests/vp_set_reference.py.  Reads the golden files only.

Bars (tests/vp_set_reference.py's header has the derivations):
  integers (counts, vp_assoc, cluster labels, which VP is split or merged, M', kept indices, flags): exact
  counts_weighted: the device adds the N weights of a VP in lanes and a reduction tree, the reference one after the other;
      every partial sum of positive terms is at most the total, so either order is within N u of the exact sum:
      |device - restatement| <= N u sum
  new VPs: residual and vector bounds of em_phase_reference.null_vector_reference against the restatement (for a merge
      widened by the bound of the row weights, which come out of an E-step and a smoothing); 1e-4 rad against the goldens
  variances: check_mstep's relative bound against the restatement; 4 x GOLDEN_S_REL relative against the goldens
"""
import ctypes
import glob
import os

import numpy as np
import pytest

from conftest import ROOT
import vp_set_reference as R
from em_phase_reference import LD, U, ld, residual, c_of_n, _ratio

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "vpset")
S_BAR = R.GOLDEN_S_FACTOR * R.GOLDEN_S_REL
EM_THRESH = 1.96 ** 2


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def names(prefix):
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


@pytest.fixture(scope="module")
def V():
    from vanishing_points_2017_amd import vp_localisation
    return vp_localisation


def angle_between(a, b):
    a, b = ld(a), ld(b)
    c = abs(np.dot(a, b)) / np.sqrt(np.dot(a, a) * np.dot(b, b))
    return float(np.arccos(min(c, LD(1))))


def check_null_vector(rec, l, r, vp, widen=LD(0)):
    """the bars em_phase_reference.check_mstep applies to the same device function"""
    s1, s2, s3 = rec["sv"]
    assert _ratio(max(residual(l, r, vp) - s3, LD(0)), rec["res_bound"] - s3 + widen) <= 1.0, "null-vector residual"
    if s2 > c_of_n(l.shape[0]) * U * s1 * 4:
        assert abs(np.sqrt(float((ld(vp) ** 2).sum())) - 1) <= 8 * float(U)
        e = np.sqrt(((ld(vp) - rec["vp"]) ** 2).sum())
        assert _ratio(e, rec["vec_bound"] + widen / (s2 - s3)) <= 1.0, "null vector"


# ---- counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("counts_"))
def test_counts(V, name):
    g = load(name)
    given = g["vp_assoc"].copy() if "vp_assoc" in g else None
    counts, cw, assoc = V.calc_vp_line_counts(g["vp"], R._lines_of(g["lp"]), g["lp"], g["s"], g["metric"], g["lweights"], "angle",
                                              thresh=float(g["thresh"]), vp_assoc=given)
    assert np.array_equal(counts, g["out_counts"]) and np.array_equal(assoc, g["out_vp_assoc"]) and assoc.dtype == np.int64
    if given is not None:
        assert np.array_equal(given, g["vp_assoc"]), "the caller's vp_assoc is not written"
    ref_cw = R.counts_reference(g["vp"], g["lp"], g["s"], g["metric"], g["lweights"], float(g["thresh"]), g.get("vp_assoc"))[1]
    print("counts_weighted error / bar:", float((np.abs(ld(cw) - ref_cw) / (g["lp"].shape[0] * U * np.maximum(ref_cw, LD(1e-300)))).max()))
    assert np.all(np.abs(ld(cw) - ref_cw) <= g["lp"].shape[0] * U * ref_cw)


def test_counts_both_thresholds_and_special_inputs(V):
    """the same lines at the reference's default 2.57 and at the EM's 1.96^2; v[2] == 0 (a NaN distance counts the
    line); zero weights; s = NaN and s < 0 (the comparison is false: the line counts)"""
    g = load("counts_n65_m2")
    for thresh in (2.57, EM_THRESH):
        got = V.calc_vp_line_counts(g["vp"], None, g["lp"], g["s"], g["metric"], g["lweights"], "angle", thresh=thresh)
        ref = R.counts_reference(g["vp"], g["lp"], g["s"], g["metric"], g["lweights"], thresh)
        assert ref[3].clear(), ref[3].worst()
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    inf = load("counts_n64_m2")                                  # (tested against its golden above: here, what it covers)
    assert inf["vp"][1, 2] == 0 and (inf["out_vp_assoc"] == 1).any(), "lines of the VP at infinity count"
    assert (g["lweights"] == 0).any() and np.all(g["out_vp_assoc"][g["lweights"] == 0] == -1)
    s = np.array([np.nan, -1.0])
    got = V.calc_vp_line_counts(g["vp"], None, g["lp"], s, g["metric"], np.ones(65), "angle")
    assert np.array_equal(got[2], np.argmax(g["metric"], axis=0)) and got[0].sum() == 65


def test_counts_tie_takes_the_first_vp(V):
    g = load("counts_n65_m2")
    metric = g["metric"].copy()
    metric[1] = metric[0]
    got = V.calc_vp_line_counts(g["vp"], None, g["lp"], np.ones(2), metric, np.ones(65), "angle", thresh=1e300)
    assert np.all(got[2] == 0) and got[0][0] == 65


def test_counts_feed_line_primitives(V):
    """calc_vp_line_counts of a foreign line set is a datum's vp_assoc for result_plotting.line_primitives"""
    from vanishing_points_2017_amd import result_plotting
    g = load("counts_n63_m2")
    counts, _, assoc = V.calc_vp_line_counts(g["vp"], None, g["lp"], g["s"], g["metric"], g["lweights"], "angle")
    datum = {"lines": {"line_segments": g["lp"]}, "EM_result": {"vp": g["vp"], "counts": counts, "vp_assoc": assoc}}
    seg, rgba, width = result_plotting.line_primitives(datum, 640, 480)[:3]
    assert seg.shape[0] == (assoc >= 0).sum() == counts.sum() and rgba.shape[0] == seg.shape[0]


# ---- split ----------------------------------------------------------------------------------------------------------------
def run_split(V, g, v=None, s=None):
    r = V.split_best_vp_batch([g["v"] if v is None else v], [g["s"] if s is None else s], [g["lp"]], [g["l"]], [g["w"]], [g["lw"]],
                              [g["langle"]], min_diff=float(g["min_diff"]))
    m = int(r["num_vp"][0])
    return r["v"].cpu().numpy()[:m], r["s"].cpu().numpy()[:m], int(r["split"][0]), int(r["flags"][0]), r["labels"].cpu().numpy()


@pytest.mark.parametrize("name", names("split_"))
def test_split(V, name):
    g = load(name)
    ref = R.split_reference(g["v"], g["s"], g["lp"], g["l"], g["w"], g["lw"], g["langle"], float(g["min_diff"]))
    v, s, split, flags, labels = run_split(V, g)
    assert split == int(g["out_split"]) and v.shape == g["out_v"].shape and flags == 0
    assert np.array_equal(labels, g["out_labels"]), "cluster labels"
    m = g["v"].shape[0]
    if split < 0:
        assert np.array_equal(v, g["v"]) and np.array_equal(s, g["s"])
        return
    keep = [k for k in range(m) if k != split]
    assert np.array_equal(v[keep], g["v"][keep]) and np.array_equal(s[keep], g["s"][keep])
    assert s[split] == g["s"][split] / 2 and s[m] == g["s"][split] / 2          # :566, one exact operation
    for rec, row in zip(ref["records"], (split, m)):
        assert angle_between(v[row], g["out_v"][row]) <= R.PARITY_RAD
        check_null_vector(rec, g["l"][rec["rows"]], g["lw"][rec["rows"]], v[row])
    assert np.all(np.abs(ld(s) - ld(g["out_s"])) <= S_BAR * np.abs(ld(g["out_s"])))


def test_split_edges_of_nworst_and_quirk(V):
    assert int(load("split_nworst8")["out_split"]) == -1 and int(load("split_nworst9")["out_split"]) >= 0
    assert int(load("split_7plus2")["out_split"]) == -1 and (load("split_7plus2")["out_labels"] == 1).sum() in (2, 7)
    assert int(load("split_too_similar")["out_split"]) == -1
    g = load("split_quirk557")
    sp = int(g["out_split"])
    assert sp >= 0 and abs(g["v"][sp, 0] / g["v"][sp, 2]) > 1 and abs(g["v"][0, 0] / g["v"][0, 2]) < 1, ":557 reads VP m"
    assert load("split_m63")["out_v"].shape[0] == 64


def test_split_overflow_leaves_the_set(V):
    g = R.split_case("split_m63", m_override=64)
    v, s, split, flags, _ = run_split(V, g)
    assert flags == V.VP_FLAG_OVERFLOW and split == -1
    assert np.array_equal(v, g["v"]) and np.array_equal(s, g["s"])


def test_split_history_slices(V):
    g = load("split_nworst9")
    m = g["v"].shape[0]
    for i in (0, 2):
        hist = np.arange(3 * m * 3, dtype=np.float64).reshape(3, m, 3) + 100
        hist[i] = g["v"]
        before, s_before = hist.copy(), g["s"].copy()
        r = V.split_best_vp(i, hist, g["s"], g["lp"], g["l"], g["w"], g["lw"], g["langle"])
        assert np.array_equal(hist, before) and np.array_equal(g["s"], s_before), "the caller's arrays are not written"
        assert r["v"].shape == (3, m + 1, 3) and r["s"].shape == (m + 1,)
        for t in range(3):
            if t != i:
                assert np.array_equal(r["v"][t, :m], before[t]) and np.all(r["v"][t, m] == 0)      # :626
        assert angle_between(r["v"][i, m], g["out_v"][m]) <= R.PARITY_RAD


def test_split_flags_disconnected_and_tie(V):
    g = load("split_nworst9")
    worst = int(g["out_split"])
    rows = np.nonzero(np.argmax(g["w"], axis=0) == worst)[0]
    mid = 0.5 * (g["lp"][rows, :2] + g["lp"][rows, 2:])
    lp = g["lp"].copy()
    lp[rows] = np.c_[mid - [0.125, 0.0], mid + [0.125, 0.0]]     # all parallel, cosines exactly 1: no distance is non-zero
    gg = dict(g, lp=lp, l=R._lines_of(lp), langle=R._fold_angles(lp))
    assert run_split(V, gg)[3] & V.VP_FLAG_SPLIT_DISCONNECTED
    dirs = np.array([[0.125, 0.0], [0.125, 0.0625], [0.0, 0.125]])[np.arange(rows.size) % 3]   # three directions, three copies
    lp[rows] = np.c_[mid - dirs, mid + dirs]
    gg = dict(g, lp=lp, l=R._lines_of(lp), langle=R._fold_angles(lp))
    assert run_split(V, gg)[3] & V.VP_FLAG_SPLIT_TIE


# ---- merge ----------------------------------------------------------------------------------------------------------------
def pdfpar_of(g):
    from vanishing_points_2017_amd.probability_functions import PDFParams
    return PDFParams(means=R._grid(), weights=g["prior_weights"], sigma=float(g["prior_sigma"]))


def run_merge(V, g, v=None, s=None, max_stdd=None):
    from vanishing_points_2017_amd.probability_functions import PDFParams
    par = PDFParams(means=None, weights=g["prior_weights"][None], sigma=float(g["prior_sigma"]))
    r = V.merge_vps_batch([g["v"] if v is None else v], [g["s"] if s is None else s], [g["l"]], float(g["thresh"]), [g["lw"]],
                          [g["lsim"]], float(g["wbias"]), par, [g["lp"]],
                          max_stdd=float(g["max_stdd"]) if max_stdd is None else max_stdd)
    m = int(r["num_vp"][0])
    return r["v"].cpu().numpy()[:m], r["s"].cpu().numpy()[:m], r["kept"].cpu().numpy()[:m], int(r["flags"][0])


@pytest.mark.parametrize("name", names("merge_"))
def test_merge(V, name):
    g = load(name)
    ref = R.merge_reference(g["v"], g["s"], g["l"], float(g["thresh"]), g["lw"], g["lsim"], float(g["wbias"]),
                            (R._grid(), g["prior_weights"], float(g["prior_sigma"])), g["lp"], float(g["max_stdd"]))
    v, s, kept, flags = run_merge(V, g)
    assert np.array_equal(kept, g["out_kept"]) and v.shape == g["out_v"].shape and flags == 0
    rounds = ref["rounds"]
    rank1 = any((not q["none"]) and q["sv"][1] <= 1e-6 * q["sv"][0] for q in rounds)
    for k in range(v.shape[0]):
        if not rank1:        # (one line: the reference's vector is LAPACK's choice in a null plane -- the residual bar below holds it)
            assert angle_between(v[k], g["out_v"][k]) <= R.PARITY_RAD
    rel = np.abs(ld(s) - ld(g["out_s"])) / np.abs(ld(g["out_s"]))
    print("s against the golden, error / bar:", float(rel.max() / S_BAR))
    assert np.all(rel <= S_BAR)
    if len(rounds) == 1:     # (later rounds start from the device's own VPs: first-order bars hold for the first)
        q = rounds[0]
        k_out = int(np.nonzero(kept == g["out_kept"][q["k"] - (1 if q["ok"] and q["j"] < q["k"] else 0)])[0][0]) if q["ok"] else q["k"]
        assert abs(LD(s[k_out]) - q["s_k"]) <= q["rel_s"] * q["s_k"], "variance of the merged VP"
        if q["ok"]:
            check_null_vector(q, g["l"], q["r"], v[k_out], widen=q["b_r"])


def test_merge_cases_are_what_they_say():
    assert load("merge_m1")["out_v"].shape[0] == 1
    assert load("merge_m2_below")["out_v"].shape[0] == 1 and load("merge_m2_above")["out_v"].shape[0] == 2
    g = load("merge_chain3")
    assert g["v"].shape[0] == 4 and list(g["out_kept"]) == [2, 3], "two rounds with a compaction between them"
    g = load("merge_abort")
    assert g["out_v"].shape[0] == 3 and (g["out_s"] != g["s"]).sum() == 1, "an aborted merge returns the changed s[k] (:666-668)"
    g = load("merge_zero_weights")
    assert g["out_v"].shape[0] == 3 and not g["lw"].any(), "newVP is None"


def test_merge_max_stdd_is_live(V):
    """the same input merges at the default 0.01 and gives up at 1e-6, the bound the EM's M-step uses"""
    g = load("merge_m2_below")
    assert run_merge(V, g, max_stdd=0.01)[0].shape[0] == 1
    ref = R.merge_reference(g["v"], g["s"], g["l"], float(g["thresh"]), g["lw"], g["lsim"], float(g["wbias"]),
                            (R._grid(), g["prior_weights"], float(g["prior_sigma"])), g["lp"], 1e-6)
    assert ref["margins"].clear() and R.merge_outcome(ref) == (0, "max_stdd")
    v, s, kept, _ = run_merge(V, g, max_stdd=1e-6)
    assert np.array_equal(v, g["v"]) and np.array_equal(kept, [0, 1]) and (s != g["s"]).sum() == 1
    k = ref["rounds"][0]["k"]
    assert abs(LD(s[k]) - ref["rounds"][0]["s_k"]) <= ref["rounds"][0]["rel_s"] * ref["rounds"][0]["s_k"]


def test_merge_identical_vps_take_the_first_pair(V):
    g = load("merge_m2_above")
    v4 = np.stack([g["v"][0], g["v"][1], g["v"][0], g["v"][1]])
    ref = R.merge_reference(v4, np.full(4, 1e-4), g["l"], float(g["thresh"]), g["lw"], g["lsim"], 1.0,
                            (R._grid(), g["prior_weights"], float(g["prior_sigma"])), g["lp"], 0.01)
    assert (ref["rounds"][0]["j"], ref["rounds"][0]["k"]) == (0, 2)
    kept = run_merge(V, g, v=v4, s=np.full(4, 1e-4))[2]
    assert np.array_equal(kept, ref["kept"])


def test_merge_history_slices(V):
    g = load("merge_chain3")
    m = g["v"].shape[0]
    llen = np.linalg.norm(g["lp"][:, :2] - g["lp"][:, 2:], axis=1)
    for i in (0, 2):
        hist = np.zeros((3, m, 3))
        hist[:, :, 0] = np.arange(m)[None, :] + 10
        hist[i] = g["v"]
        before, s_before = hist.copy(), g["s"].copy()
        r = V.merge_vps(i, hist, g["s"], g["l"], float(g["thresh"]), g["lw"], g["lsim"], 1, pdfpar_of(g), g["lp"], llen, "angle")
        assert np.array_equal(hist, before) and np.array_equal(g["s"], s_before), "the caller's arrays are not written"
        assert r["v"].shape == (3, 2, 3) and r["s"].shape == (2,)
        for t in range(3):
            if t != i:
                assert np.array_equal(r["v"][t, :, 0], g["out_kept"] + 10)                 # :674 deletes the column everywhere
        for k in range(2):
            assert angle_between(r["v"][i, k], g["out_v"][k]) <= R.PARITY_RAD


# ---- batches --------------------------------------------------------------------------------------------------------------
BATCH_N = (0, 1, 12, 65, 130)


def same_bits(a, b):
    """bit for bit, NaNs included (with one line on another VP, s[k] of a merge is log(0) - log(0))"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def images():
    out = []
    for q, n in enumerate(BATCH_N):
        rs = np.random.RandomState(500 + q)
        base, pts = R._vps_in_image(rs, 2)
        v = np.stack([base[0], base[1], R._rotate(base[0], 2e-4, rs)])
        own = rs.randint(0, 2, n)
        lp = np.concatenate([R._segments_to(rs, pts[own[i]], 1, 0.15) for i in range(n)]) if n else np.zeros((0, 4))
        out.append({"v": v, "s": np.full(3, 1e-4), "lp": lp, "l": R._lines_of(lp) if n else np.zeros((0, 3)),
                    "metric": rs.rand(3, n), "lw": rs.uniform(0.2, 1.0, n), "cnn": rs.rand(20, 20).astype(np.float32) ** 4})
    return out


def test_batch_equals_single_calls(V, images):
    from vanishing_points_2017_amd import probability_functions as P
    key = lambda k: [im[k] for im in images]
    c, cw, a, lo, vo = V.calc_vp_line_counts_batch(key("v"), key("lp"), key("s"), key("metric"), key("lw"), thresh=1e-3)
    c, cw, a = c.cpu().numpy(), cw.cpu().numpy(), a.cpu().numpy()
    assert list(np.diff(lo)) == list(BATCH_N)
    lsims = V.calc_lsim_batch(key("lp"), sigma=1)
    lscore, langle, llen, _ = V.line_geometry_batch(key("lp"), k1=10, k2=4, sigma=1)
    par = P.pdf_params_batch(np.stack(key("cnn")))
    mb = V.merge_vps_batch(key("v"), key("s"), key("l"), 1e-3, key("lw"), lsims, 1, par, key("lp"))
    la = langle.cpu().numpy()
    sb = V.split_best_vp_batch(key("v"), key("s"), key("lp"), key("l"), key("metric"), key("lw"),
                               [la[lo[b]:lo[b + 1]] for b in range(5)])
    for b, im in enumerate(images):
        if BATCH_N[b] == 0:
            assert not c[vo[b]:vo[b + 1]].any() and np.array_equal(mb["v"].cpu().numpy()[vo[b]:vo[b + 1]], im["v"])
            assert int(sb["num_vp"][b]) == 3 and int(sb["split"][b]) == -1
            continue
        one = V.calc_vp_line_counts(im["v"], None, im["lp"], im["s"], im["metric"], im["lw"], "angle", thresh=1e-3)
        assert np.array_equal(one[0], c[vo[b]:vo[b + 1]]) and np.array_equal(one[1], cw[vo[b]:vo[b + 1]])
        assert np.array_equal(one[2], a[lo[b]:lo[b + 1]])
        par1 = P.pdf_params(im["cnn"])
        lsim1 = V.calc_lsim(im["lp"], sigma=1)
        assert np.array_equal(lsim1, lsims[b].cpu().numpy())
        one = V.merge_vps(0, im["v"][None], im["s"], im["l"], 1e-3, im["lw"], lsim1, 1, par1, im["lp"], None, "angle")
        m = int(mb["num_vp"][b])
        assert one["v"].shape[1] == m
        assert same_bits(one["v"][0], mb["v"].cpu().numpy()[vo[b]:vo[b] + m])
        assert same_bits(one["s"], mb["s"].cpu().numpy()[vo[b]:vo[b] + m])
        one = V.split_best_vp(0, im["v"][None], im["s"], im["lp"], im["l"], im["metric"], im["lw"], la[lo[b]:lo[b + 1]])
        m = int(sb["num_vp"][b])
        o0 = int(sb["out_offsets"][b])
        assert one["v"].shape[1] == m and same_bits(one["v"][0], sb["v"].cpu().numpy()[o0:o0 + m])


def test_device_composed_merge_equals_host_inputs(V, images):
    """pdf_params_batch + calc_lsim_batch + line_geometry_batch -> merge_vps_batch without a host copy, against the same
    call on host arrays: bit for bit"""
    import torch
    from vanishing_points_2017_amd import probability_functions as P
    key = lambda k: [im[k] for im in images]
    dev = torch.device("cuda", 0)
    lo = np.concatenate(([0], np.cumsum(BATCH_N))).astype(np.int64)
    vo = np.arange(6, dtype=np.int64) * 3
    d_lp = torch.from_numpy(np.concatenate(key("lp"))).to(dev)
    d_l = torch.from_numpy(np.concatenate(key("l"))).to(dev)
    d_v = torch.from_numpy(np.concatenate(key("v"))).to(dev)
    d_s = torch.from_numpy(np.concatenate(key("s"))).to(dev)
    d_maps = torch.from_numpy(np.stack(key("cnn"))).to(dev)
    lscore, langle, llen, off = V.line_geometry_batch((d_lp, lo), k1=10, k2=4, sigma=1)
    lsims = V.calc_lsim_batch((d_lp, lo), sigma=1)
    par = P.pdf_params_batch(d_maps)
    d_lw = llen * lscore.clamp(0.2, 1.0)                         # lweight as the EM's set-up makes it (:227-233)
    r = V.merge_vps_batch(d_v, d_s, d_l, 1e-3, d_lw, lsims, 1, par, d_lp, line_offsets=off, vp_offsets=vo)
    lw = d_lw.cpu().numpy()
    h = V.merge_vps_batch(key("v"), key("s"), key("l"), 1e-3, [lw[lo[b]:lo[b + 1]] for b in range(5)],
                          [x.cpu().numpy() for x in lsims], 1,
                          P.PDFParams(means=None, weights=par.weights.cpu().numpy(), sigma=par.sigma), key("lp"))
    for k in ("v", "s", "num_vp", "kept", "flags"):
        assert same_bits(r[k].cpu().numpy(), h[k].cpu().numpy()), k


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_errors_touch_nothing_and_ranges_hold(V, images):
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    t = rt.torch
    key = lambda k: [im[k] for im in images]
    lo = np.concatenate(([0], np.cumsum(BATCH_N))).astype(np.int64)
    vo = np.arange(6, dtype=np.int64) * 3
    P_ = lambda a: ctypes.c_void_p(a.ctypes.data)
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(rt.tdev)
    lp, v, s, lw = up(np.concatenate(key("lp"))), up(np.concatenate(key("v"))), up(np.concatenate(key("s"))), up(np.concatenate(key("lw")))
    w = up(np.concatenate([im["metric"].ravel() for im in images]))
    SENT = -7.0
    counts = t.full((15 + 4,), SENT, dtype=t.float64, device=rt.tdev)
    cw = t.full((15 + 4,), SENT, dtype=t.float64, device=rt.tdev)
    assoc = t.full((int(lo[-1]) + 4,), -7, dtype=t.int64, device=rt.tdev)

    def call(batch, lo_, vo_, lp_=lp, out=counts):
        rc = rt.lib.vpk_vp_line_counts_batch(rt.h, batch, lo_, vo_, rt.ptr(lp_), rt.ptr(v), rt.ptr(s), rt.ptr(w), rt.ptr(lw), 1e-3, None,
                                             rt.ptr(out), rt.ptr(cw), rt.ptr(assoc))
        rt.synchronize()
        return rc

    untouched = lambda: bool((counts == SENT).all()) and bool((cw == SENT).all()) and bool((assoc == -7).all())
    with rt.on_stream():
        assert call(0, None, None) == 0 and untouched(), "batch = 0 does nothing"
        assert call(-1, P_(lo), P_(vo)) == -1 and untouched()
        assert call(5, None, P_(vo)) == -1 and untouched()
        bad = lo.copy(); bad[2] = 0; bad[1] = 5
        assert call(5, P_(bad), P_(vo)) == -1 and untouched(), "offsets that decrease"
        assert call(5, P_(lo), P_(vo), lp_=None) == -1 and untouched(), "null buffer"
        big, one = np.array([0, 65], dtype=np.int64), np.array([0, 65], dtype=np.int64)
        assert call(1, P_(one), P_(big)) == -5 and untouched(), "VPK_ERR_LIMIT before any launch"
        N9 = [None] * 9
        assert rt.lib.vpk_vp_split_batch(rt.h, -1, *N9, 1e-4, *([None] * 6)) == -1
        assert rt.lib.vpk_vp_split_batch(rt.h, 5, P_(lo), None, *([None] * 7), 1e-4, *([None] * 6)) == -1
        assert rt.lib.vpk_vp_split_batch(rt.h, 0, *N9, 1e-4, *([None] * 6)) == 0
        assert rt.lib.vpk_vp_merge_batch(rt.h, -1, *N9, 1.0, None, 1.0, 1e-3, 0.01, *([None] * 5)) == -1
        assert rt.lib.vpk_vp_merge_batch(rt.h, 0, *N9, 1.0, None, 1.0, 1e-3, 0.01, *([None] * 5)) == 0
        # merge: lsim_offsets that leave an image less than N^2 elements, and more than 64 VPs, with real outputs
        short = np.zeros(6, dtype=np.int64)
        l3 = up(np.concatenate(key("l")))
        pw = t.zeros((5, 400), dtype=t.float32, device=rt.tdev)
        num = t.full((5,), -7, dtype=t.int32, device=rt.tdev)
        mo = lambda lo_, vo_, lso: rt.lib.vpk_vp_merge_batch(rt.h, len(lo_) - 1, P_(lo_), P_(vo_), rt.ptr(lp), rt.ptr(l3), rt.ptr(v), rt.ptr(s),
                                                            rt.ptr(lw), P_(lso), rt.ptr(w), 1.0, rt.ptr(pw), 0.1, 1e-3, 0.01, rt.ptr(counts),
                                                            rt.ptr(cw), rt.ptr(num), rt.ptr(num), rt.ptr(num))
        assert mo(lo, vo, short) == -1
        assert mo(np.array([0, 1], dtype=np.int64), big, np.array([0, 1], dtype=np.int64)) == -5
        rt.synchronize()
        assert untouched() and bool((num == -7).all())
        assert call(5, P_(lo), P_(vo)) == 0
    c = counts.cpu().numpy()
    assert (c[:3] == SENT).all() and (c[15:] == SENT).all() and (c[3:15] != SENT).all(), "the image without lines and the tail are not written"
    assert (cw.cpu().numpy()[15:] == SENT).all() and (assoc.cpu().numpy()[int(lo[-1]):] == -7).all()
    assert (assoc.cpu().numpy()[:int(lo[-1])] != -7).all()
