"""calc_vp_line_counts_batch and merge_vps_batch under "dotprod" and "area" on the GPU (vpk_vp_line_counts_batch_measure,
vpk_vp_merge_batch_measure) held to the reference's recorded results (tests/golden/vpset_measures) and to the
extended-precision restatements of tests/vp_set_measure_reference.py.  Reads the golden files only.  CPU twin:
tests/test_vp_set_measures.py (the host build of the same device code, the same bars).

Bars (tests/vp_set_measure_reference.py's and tests/vp_set_reference.py's headers have the derivations):
  integers (counts, vp_assoc, which VPs are merged, M', kept indices, flags): exact
  counts_weighted: |device - restatement| <= N u sum (lanes and a reduction tree against a running sum of positive terms)
  new VPs: null_vector_reference's residual and vector bounds against the restatement, widened by the bound of the row
      weights under the measure; 1e-4 rad against the goldens
  variances: check_mstep's relative bound, widened by the E-step's bounds under the measure, against the restatement;
      GOLDEN_S_FACTOR x GOLDEN_S_REL[measure] relative against the goldens (measured on the CPU, never on the device)
"""
import ctypes
import os

import numpy as np
import pytest

import vp_set_reference as R
import vp_set_measure_reference as RM
from em_phase_reference import LD
from vp_set_measure_reference import COUNTS, check_counts, check_merge

pytestmark = pytest.mark.gpu

ALL = ("angle",) + RM.MEASURES
CODE = {"angle": 0, "dotprod": 1, "area": 2}
EM_THRESH = 1.96 ** 2


@pytest.fixture(scope="module")
def V():
    from vanishing_points_2017_amd import vp_localisation
    return vp_localisation


def _np(x):
    return x.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_counts(V, measure, vp, lp, l, s, metric, lw, thresh=2.57, vp_assoc=None):
    c, cw, a, _, _ = V.calc_vp_line_counts_batch([vp], [lp], [s], None if metric is None else [metric], [lw], measure, thresh,
                                                 None if vp_assoc is None else [vp_assoc], ls=[l] if measure == "dotprod" else None)
    return _np(c), _np(cw), _np(a)


def run_merge(V, measure, g, max_stdd=None):
    from vanishing_points_2017_amd.probability_functions import PDFParams
    par = PDFParams(means=None, weights=g["prior_weights"][None], sigma=float(g["prior_sigma"]))
    r = V.merge_vps_batch([g["v"]], [g["s"]], [g["l"]], float(g["thresh"]), [g["lw"]], [g["lsim"]], float(g["wbias"]), par, [g["lp"]],
                          distance_measure=measure, max_stdd=float(g["max_stdd"]) if max_stdd is None else max_stdd)
    m = int(r["num_vp"][0])
    return _np(r["v"])[:m], _np(r["s"])[:m], _np(r["kept"])[:m], int(r["flags"][0])


# ---- 1: counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure,name", [(m, n) for m in RM.MEASURES for n in COUNTS])
def test_counts(V, measure, name):
    g = RM.golden(measure, name)
    given = g["vp_assoc"].copy() if "vp_assoc" in g else None
    got = run_counts(V, measure, g["vp"], g["lp"], g["l"], g["s"], g["metric"], g["lweights"], float(g["thresh"]), given)
    check_counts(got, measure, g)
    if given is not None:
        assert np.array_equal(given, g["vp_assoc"]), "the caller's vp_assoc is not written"


# ---- 2: special inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", RM.MEASURES)
def test_counts_special_inputs(V, measure):
    """v[2] == 0 (NaN under "area", finite under "dotprod"); zero weights; s = NaN and s < 0 (the comparison is false: the
    line counts); both thresholds on the same lines -- each against the restatement"""
    g = RM.golden(measure, "counts_n65_m2")
    assert g["vp"][1, 2] == 0 and (g["lweights"] == 0).any()
    assoc = np.arange(65, dtype=np.int64) % 2                    # every other line on the VP at infinity
    for thresh in (2.57, EM_THRESH):
        for given in (None, assoc):
            got = run_counts(V, measure, g["vp"], g["lp"], g["l"], g["s"], g["metric"], g["lweights"], thresh, given)
            ref = RM.counts_reference(measure, g["vp"], g["lp"], g["l"], g["s"], g["metric"], g["lweights"], thresh, given)
            assert ref[3].clear(), ref[3].worst()
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
            assert np.all(got[2][g["lweights"] == 0] == -1)
        if measure == "area":                                     # a NaN distance: every line of that VP counts, unless its weight is 0
            assert np.array_equal(got[2] == 1, (assoc == 1) & (g["lweights"] != 0))
        else:                                                     # finite at infinity: :504 decides
            assert 0 < (got[2] == 1).sum() < ((assoc == 1) & (g["lweights"] != 0)).sum()
    s = np.array([np.nan, -1.0])
    for given in (None, assoc):
        got = run_counts(V, measure, g["vp"], g["lp"], g["l"], s, g["metric"], np.ones(65), 2.57, given)
        ref = RM.counts_reference(measure, g["vp"], g["lp"], g["l"], s, g["metric"], np.ones(65), 2.57, given)
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[0], ref[0])
        assert np.array_equal(got[2], np.argmax(g["metric"], axis=0) if given is None else assoc) and got[0].sum() == 65


def test_counts_area_negative_radicand_counts_the_line(V):
    """c^2 < b^2 (:245): at right angles to the VP's direction the radicand is negative through rounding, the distance NaN
    and :504 false"""
    vp, lp = RM.negative_radicand_case()
    n = lp.shape[0]
    assoc = np.zeros(n, dtype=np.int64)
    ref = RM.counts_reference("area", vp, lp, None, np.array([1e-12]), None, np.ones(n), 2.57, assoc)
    got = run_counts(V, "area", vp, lp, None, np.array([1e-12]), None, np.ones(n), 2.57, assoc)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and got[0][0] == n
    # (the same lines against a VP that is not at right angles are outliers at this s: the test above is not vacuous)
    other = R._unit([[vp[0, 1], -vp[0, 0] + 0.3, vp[0, 2]]])
    ref = RM.counts_reference("area", other, lp, None, np.array([1e-12]), None, np.ones(n), 2.57, assoc)
    got = run_counts(V, "area", other, lp, None, np.array([1e-12]), None, np.ones(n), 2.57, assoc)
    assert ref[3].clear() and np.array_equal(got[0], ref[0]) and got[0][0] < n


# ---- 3: merge -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure,name", [(m, n) for m in RM.MEASURES for n in sorted(R.MERGE_SPECS)])
def test_merge(V, measure, name):
    g = RM.golden(measure, name)
    check_merge(run_merge(V, measure, g), measure, g, RM.merge_reference_of(measure, g))


def test_merge_gives_up_where_the_measure_says(V):
    """at the default 0.01 the pair merges under every measure; "dotprod" gives up at 1e-3 already, "area" at 1e-6"""
    for measure, low in (("dotprod", 1e-3), ("area", 1e-6)):
        g = RM.golden(measure, "merge_m2_below")
        assert run_merge(V, measure, g, max_stdd=0.01)[0].shape[0] == 1
        ref = RM.merge_reference(measure, g["v"], g["s"], g["l"], float(g["thresh"]), g["lw"], g["lsim"], float(g["wbias"]),
                                 RM.pdfpar_of(g), g["lp"], low)
        assert ref["margins"].clear() and R.merge_outcome(ref) == (0, "max_stdd")
        v, s, kept, _ = run_merge(V, measure, g, max_stdd=low)
        assert np.array_equal(v, g["v"]) and np.array_equal(kept, [0, 1]) and (s != g["s"]).sum() == 1
        q = ref["rounds"][0]
        assert abs(LD(s[q["k"]]) - q["s_k"]) <= q["rel_s"] * q["s_k"]


# ---- 4: batches -----------------------------------------------------------------------------------------------------------
BATCH_N = (12, 0, 130, 1, 65)
BATCH_M = (3, 3, 3, 0, 3)


@pytest.fixture(scope="module")
def images():
    out = []
    for q, (n, m) in enumerate(zip(BATCH_N, BATCH_M)):
        rs = np.random.RandomState(700 + q)
        base, pts = R._vps_in_image(rs, 2)
        v = np.stack([base[0], base[1], R._rotate(base[0], 2e-4, rs)])[:m].reshape(m, 3)
        own = rs.randint(0, 2, n)
        lp = np.concatenate([R._segments_to(rs, pts[own[i]], 1, 0.15) for i in range(n)]) if n else np.zeros((0, 4))
        out.append({"v": v, "s": np.full(m, 1e-4), "lp": lp, "l": R._lines_of(lp) if n else np.zeros((0, 3)),
                    "metric": rs.rand(m, n), "lw": rs.uniform(0.2, 1.0, n), "cnn": rs.rand(20, 20).astype(np.float32) ** 4})
    return out


COUNT_THRESH = {"angle": 1e-3, "dotprod": 2.57, "area": 1e-3}     # some lines inside, some outside, at s = 1e-4


@pytest.mark.parametrize("measure", ALL)
def test_batch_equals_one_image_launches_and_device_inputs_equal_host_lists(V, images, measure):
    import torch
    from vanishing_points_2017_amd import probability_functions as P
    key = lambda k: [im[k] for im in images]
    thresh = COUNT_THRESH[measure]
    c, cw, a, lo, vo = V.calc_vp_line_counts_batch(key("v"), key("lp"), key("s"), key("metric"), key("lw"), measure, thresh, ls=key("l"))
    c, cw, a = _np(c), _np(cw), _np(a)
    assert list(np.diff(lo)) == list(BATCH_N) and list(np.diff(vo)) == list(BATCH_M)
    assert 0 < c.sum() < sum(n for n, m in zip(BATCH_N, BATCH_M) if m), "lines inside and outside the threshold"
    lsims = V.calc_lsim_batch(key("lp"), sigma=1)
    par = P.pdf_params_batch(np.stack(key("cnn")))
    mb = V.merge_vps_batch(key("v"), key("s"), key("l"), 1e-3, key("lw"), lsims, 1, par, key("lp"), distance_measure=measure)
    merged = 0
    for b, im in enumerate(images):
        n, m = BATCH_N[b], BATCH_M[b]
        if n == 0 or m == 0:
            assert not c[vo[b]:vo[b + 1]].any() and np.all(a[lo[b]:lo[b + 1]] == -1)
            assert int(mb["num_vp"][b]) == m and same_bits(_np(mb["v"])[vo[b]:vo[b + 1]], im["v"])
            continue
        one = run_counts(V, measure, im["v"], im["lp"], im["l"], im["s"], im["metric"], im["lw"], thresh)
        assert same_bits(one[0], c[vo[b]:vo[b + 1]]) and same_bits(one[1], cw[vo[b]:vo[b + 1]]) and same_bits(one[2], a[lo[b]:lo[b + 1]])
        par1 = P.PDFParams(means=None, weights=_np(par.weights)[b:b + 1], sigma=par.sigma)
        r1 = V.merge_vps_batch([im["v"]], [im["s"]], [im["l"]], 1e-3, [im["lw"]], [_np(lsims[b])], 1, par1, [im["lp"]],
                               distance_measure=measure)
        k = int(mb["num_vp"][b])
        assert int(r1["num_vp"][0]) == k and int(r1["flags"][0]) == int(mb["flags"][b])
        for f in ("v", "s", "kept"):
            assert same_bits(_np(r1[f])[:k], _np(mb[f])[vo[b]:vo[b] + k]), f
        merged += m - k
    assert merged > 0, "a merge was carried out"
    # device tensors with offsets against the host lists
    dev = torch.device("cuda", 0)
    up = lambda k, shape: torch.from_numpy(np.concatenate([im[k].reshape(shape) for im in images])).to(dev)
    d_lp, d_l, d_v, d_s, d_lw = up("lp", (-1, 4)), up("l", (-1, 3)), up("v", (-1, 3)), up("s", (-1,)), up("lw", (-1,))
    d_w = up("metric", (-1,))
    dc, dcw, da, _, _ = V.calc_vp_line_counts_batch(d_v, d_lp, d_s, d_w, d_lw, measure, thresh, line_offsets=lo, vp_offsets=vo, ls=d_l)
    assert same_bits(_np(dc), c) and same_bits(_np(dcw), cw) and same_bits(_np(da), a)
    dm = V.merge_vps_batch(d_v, d_s, d_l, 1e-3, d_lw, lsims, 1, par, d_lp, distance_measure=measure, line_offsets=lo, vp_offsets=vo)
    for f in ("v", "s", "num_vp", "kept", "flags"):
        assert same_bits(_np(dm[f]), _np(mb[f])), f


# ---- 5: "angle" through the new entry points is the old entry points ------------------------------------------------------
def _old_golden(name):
    with np.load(os.path.join(os.path.dirname(RM.GOLDEN), "vpset", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def test_angle_through_the_new_entries_is_the_old_entries(V):
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    t = rt.torch
    up = lambda x, dt=np.float64: t.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(rt.tdev)
    P_ = lambda x: ctypes.c_void_p(x.ctypes.data)
    for name in ("counts_n63_m2", "counts_n65_m64", "counts_n513_m1", "counts_n513_m64"):
        g = _old_golden(name)
        n, m = g["lp"].shape[0], g["vp"].shape[0]
        lo, vo = np.array([0, n], dtype=np.int64), np.array([0, m], dtype=np.int64)
        lp, v, s, w, lw = up(g["lp"]), up(g["vp"]), up(g["s"]), up(g["metric"]), up(g["lweights"])
        ain = up(g["vp_assoc"], np.int64) if "vp_assoc" in g else None
        out = []
        for new in (False, True):
            c, cw = t.zeros(m, dtype=t.float64, device=rt.tdev), t.zeros(m, dtype=t.float64, device=rt.tdev)
            a = t.full((n,), -1, dtype=t.int64, device=rt.tdev)
            with rt.on_stream():
                if new:
                    rc = rt.lib.vpk_vp_line_counts_batch_measure(rt.h, 0, 1, P_(lo), P_(vo), rt.ptr(lp), None, rt.ptr(v), rt.ptr(s),
                                                                 rt.ptr(w), rt.ptr(lw), float(g["thresh"]), rt.ptr(ain), rt.ptr(c),
                                                                 rt.ptr(cw), rt.ptr(a))
                else:
                    rc = rt.lib.vpk_vp_line_counts_batch(rt.h, 1, P_(lo), P_(vo), rt.ptr(lp), rt.ptr(v), rt.ptr(s), rt.ptr(w), rt.ptr(lw),
                                                         float(g["thresh"]), rt.ptr(ain), rt.ptr(c), rt.ptr(cw), rt.ptr(a))
            rt.synchronize()
            assert rc == 0
            out.append((_np(c), _np(cw), _np(a)))
        assert all(same_bits(x, y) for x, y in zip(*out)), name
        assert np.array_equal(out[1][0], g["out_counts"]) and np.array_equal(out[1][2], g["out_vp_assoc"])
    for name in ("merge_chain3", "merge_abort", "merge_n65"):
        g = _old_golden(name)
        n, m = g["lp"].shape[0], g["v"].shape[0]
        lo, vo, so = np.array([0, n], dtype=np.int64), np.array([0, m], dtype=np.int64), np.array([0, n * n], dtype=np.int64)
        lp, l, v, s, lw, lsim = up(g["lp"]), up(g["l"]), up(g["v"]), up(g["s"]), up(g["lw"]), up(g["lsim"])
        pw = up(g["prior_weights"], np.float32)
        out = []
        for new in (False, True):
            vo_, so_ = t.zeros((m, 3), dtype=t.float64, device=rt.tdev), t.zeros(m, dtype=t.float64, device=rt.tdev)
            num, fl = t.zeros(1, dtype=t.int32, device=rt.tdev), t.zeros(1, dtype=t.int32, device=rt.tdev)
            keep = t.zeros(m, dtype=t.int32, device=rt.tdev)
            tail = (rt.ptr(lp), rt.ptr(l), rt.ptr(v), rt.ptr(s), rt.ptr(lw), P_(so), rt.ptr(lsim), float(g["wbias"]), rt.ptr(pw),
                    float(g["prior_sigma"]), float(g["thresh"]), float(g["max_stdd"]), rt.ptr(vo_), rt.ptr(so_), rt.ptr(num),
                    rt.ptr(keep), rt.ptr(fl))
            with rt.on_stream():
                rc = rt.lib.vpk_vp_merge_batch_measure(rt.h, 0, 1, P_(lo), P_(vo), *tail) if new else \
                    rt.lib.vpk_vp_merge_batch(rt.h, 1, P_(lo), P_(vo), *tail)
            rt.synchronize()
            assert rc == 0
            out.append(tuple(_np(x) for x in (vo_, so_, num, keep, fl)))
        assert all(same_bits(x, y) for x, y in zip(*out)), name
        k = int(out[1][2][0])
        assert np.array_equal(out[1][3][:k], g["out_kept"])


# ---- 6: a composed iteration, counts under the chain's own measure and a merge behind it -------------------------------------
def _chain(measure, host):
    """tests/test_gpu_emstep.py's chain -- prior, E-step, weights, M-step, counts -- with the count step under ``measure``
    and a merge of the M-step's set after it.  host: every stage is fed host copies of the previous stage's output."""
    import torch
    from golden_util import load
    from oracle import em_numpy as em
    from vanishing_points_2017_amd import probability_functions as P
    from vanishing_points_2017_amd import vp_localisation as V
    from vanishing_points_2017_amd.runtime import get_runtime
    dev = get_runtime(0).tdev
    gs = [load(name) for name in ("clean3_n60", "tiny_n12", "yud_n120")]
    for g in gs:
        g["lnorm"] = g["l"] / np.sqrt((g["l"] ** 2).sum(1))[:, None]
    maps = np.stack([g["cnn_response"] for g in gs])
    spheres = np.stack([g["sphere_image"] for g in gs])
    lps = [torch.from_numpy(np.ascontiguousarray(g["lp"], dtype=np.float64)).to(dev) for g in gs]
    ls = [torch.from_numpy(np.ascontiguousarray(g["lnorm"])).to(dev) for g in gs]
    off = np.concatenate(([0], np.cumsum([g["lp"].shape[0] for g in gs]))).astype(np.int64)
    pair = (torch.cat(lps), off)

    def hop(x):
        if not host:
            assert all(t.is_cuda for t in (x if isinstance(x, list) else [x]))
            return x
        return [_np(t) for t in x] if isinstance(x, list) else _np(x)

    lsims = V.calc_lsim_batch(pair, sigma=1)
    lscore, langle, llen, off = V.line_geometry_batch(pair, k1=10, k2=4)
    lw = hop(llen * lscore.clamp(0.2, 1))
    v0, num = V.find_initial_vps_batch(spheres, maps, 25)
    vs = hop([v0[b, :k] for b, k in enumerate(num.tolist())])
    s0 = (np.pi / (1.282 * 20)) * (1e-3 if measure == "dotprod" else 1e-6)     # :196-201
    ss = [np.full(len(v), s0) for v in vs]
    e = P.calc_probabilities_batch(maps, vs, ls, lps, ss, distance_measure=measure)
    p_vl, lvsq = hop([p.vl for p in e['pdf']]), hop([p.lvsq for p in e['pdf']])
    w = hop(V.weight_matrix_batch(p_vl, lw, hop(lsims), bias=1, line_offsets=off))
    r = V.mstep_batch(ls, w, lvsq, p_vl, vs, max_stdd=1e-3 if measure == "dotprod" else 1e-6, s_thresh=1e-200)
    l_cat = hop(torch.cat(ls))
    counts, counts_w, assoc, _, _ = V.calc_vp_line_counts_batch(hop(r['v']), pair[0], hop(r['s']), w, lw, measure, EM_THRESH,
                                                                line_offsets=off, vp_offsets=r['vp_offsets'], ls=l_cat)
    par = P.pdf_params_batch(maps)
    if host:
        par = P.PDFParams(means=None, weights=_np(par.weights), sigma=par.sigma)
    mg = V.merge_vps_batch(hop(r['v']), hop(r['s']), l_cat, 1e-2, lw, hop(lsims), 1, par, pair[0], distance_measure=measure,
                           line_offsets=off, vp_offsets=r['vp_offsets'])
    out = {"counts": _np(counts), "counts_w": _np(counts_w), "assoc": _np(assoc)}
    out.update({"merge_" + k: _np(mg[k]) for k in ("v", "s", "num_vp", "kept", "flags")})
    out.update({"mstep_" + k: _np(r[k]) for k in ("v", "s", "removed")})
    return out


@pytest.mark.parametrize("measure", RM.MEASURES)
def test_composed_iteration_counts_and_merges_under_its_own_measure(measure):
    dev, hst = _chain(measure, False), _chain(measure, True)
    for k in dev:
        assert same_bits(dev[k], hst[k]), k
    assert dev["counts"].sum() > 0, "the count step found inliers under its measure"


# ---- 7: the EM's own decisions under "dotprod" ----------------------------------------------------------------------------
def _em_stems():
    from em_dotprod_cases import stems
    return stems()


@pytest.mark.parametrize("stem", _em_stems())
def test_counts_reproduce_the_em_under_dotprod(V, stem):
    """the stand-alone counts on the EM's final VPs, variances and decision metric are the EM's own counts and vp_assoc
    (:417-418): the recorder kept only scenes with no line within 1e-9 of its threshold"""
    from em_dotprod_cases import scene
    from vanishing_points_2017_amd import em as gem
    sc, kw = scene(stem)
    res = gem.em_batch([sc], want_metric=True, distance_measure="dotprod", **kw)[0]
    assert res["status"] == 0
    n = sc["lp"].shape[0]
    if kw.get("use_weights", True):
        lscore, _, llen, _ = V.line_geometry_batch([sc["lp"]], k1=10, k2=4)
        lw = _np(llen * lscore.clamp(0.2, 1))
    else:
        lw = np.ones(n)
    got = run_counts(V, "dotprod", res["vp"], sc["lp"], res["l"], res["sigma"], res["decision_metric"], lw,
                     kw.get("outlier_thresh", EM_THRESH))
    assert np.array_equal(got[0], res["counts"]) and np.array_equal(got[2], res["vp_assoc"])


# ---- 8: C ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_errors_touch_nothing(V, images):
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    t = rt.torch
    key = lambda k: [im[k] for im in images]
    lo = np.concatenate(([0], np.cumsum(BATCH_N))).astype(np.int64)
    vo = np.concatenate(([0], np.cumsum(BATCH_M))).astype(np.int64)
    P_ = lambda a: ctypes.c_void_p(a.ctypes.data)
    up = lambda a, dt=np.float64: t.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(rt.tdev)
    lp, l, v, s, lw = (up(np.concatenate(key(k))) for k in ("lp", "l", "v", "s", "lw"))
    w = up(np.concatenate([im["metric"].ravel() for im in images]))
    lsim_off = np.concatenate(([0], np.cumsum(np.array(BATCH_N) ** 2))).astype(np.int64)
    lsim = t.zeros((int(lsim_off[-1]),), dtype=t.float64, device=rt.tdev)
    pw = t.zeros((5, 400), dtype=t.float32, device=rt.tdev)
    SENT = -7.0
    nm, nl = int(vo[-1]), int(lo[-1])
    counts, cw = t.full((nm,), SENT, dtype=t.float64, device=rt.tdev), t.full((nm,), SENT, dtype=t.float64, device=rt.tdev)
    assoc = t.full((nl,), -7, dtype=t.int64, device=rt.tdev)
    v_out, s_out = t.full((nm, 3), SENT, dtype=t.float64, device=rt.tdev), t.full((nm,), SENT, dtype=t.float64, device=rt.tdev)
    num, keep, fl = (t.full((k,), -7, dtype=t.int32, device=rt.tdev) for k in (5, nm, 5))

    def cnt(measure, batch, l_=l, lo_=lo, vo_=vo):
        rc = rt.lib.vpk_vp_line_counts_batch_measure(rt.h, measure, batch, None if lo_ is None else P_(lo_), None if vo_ is None else P_(vo_),
                                                     rt.ptr(lp), rt.ptr(l_), rt.ptr(v), rt.ptr(s), rt.ptr(w), rt.ptr(lw), 2.57, None,
                                                     rt.ptr(counts), rt.ptr(cw), rt.ptr(assoc))
        rt.synchronize()
        return rc

    def mrg(measure, batch, lo_=lo, vo_=vo):
        rc = rt.lib.vpk_vp_merge_batch_measure(rt.h, measure, batch, None if lo_ is None else P_(lo_), None if vo_ is None else P_(vo_),
                                               rt.ptr(lp), rt.ptr(l), rt.ptr(v), rt.ptr(s), rt.ptr(lw), P_(lsim_off), rt.ptr(lsim), 1.0,
                                               rt.ptr(pw), 0.1, 1e-3, 0.01, rt.ptr(v_out), rt.ptr(s_out), rt.ptr(num), rt.ptr(keep),
                                               rt.ptr(fl))
        rt.synchronize()
        return rc

    def untouched():
        return all(bool((x == SENT).all()) for x in (counts, cw, v_out, s_out)) and bool((assoc == -7).all()) and \
            all(bool((x == -7).all()) for x in (num, keep, fl))

    with rt.on_stream():
        for bad in (3, -1, 17):
            assert cnt(bad, 5) == -1 and mrg(bad, 5) == -1 and untouched(), "unknown measure"
        assert cnt(1, 5, l_=None) == -1 and untouched(), "\"dotprod\" with l NULL"
        for measure in (0, 1, 2):
            assert cnt(measure, -1) == -1 and mrg(measure, -1) == -1 and untouched(), "batch < 0"
            assert cnt(measure, 0, lo_=None, vo_=None) == 0 and mrg(measure, 0, lo_=None, vo_=None) == 0 and untouched(), "batch = 0"
            assert cnt(measure, 5, lo_=None) == -1 and mrg(measure, 5, vo_=None) == -1 and untouched()
        assert cnt(0, 5, l_=None) == 0 and cnt(2, 5, l_=None) == 0, "l may be NULL unless the measure reads it"
        assert cnt(1, 5) == 0 and mrg(2, 5) == 0
    c = _np(counts)
    for b in range(5):
        written = BATCH_N[b] > 0 and BATCH_M[b] > 0
        assert np.all((c[vo[b]:vo[b + 1]] != SENT) == written), "an image without lines or VPs is not written"
        assert bool((num[b] != -7)) == written
