"""vpk_estep_batch (csrc/vpk_estep.hip) and the E-step call surface of probability_functions on top of it, against the
reference's stored output (tests/golden/estep/) and the extended-precision restatement (tests/estep_reference.py, which
derives every bound).

Shapes: a workgroup covers 64 lines of one image and stages 128 VPs at a time, so N = 1, 63, 64, 65 and 130 (one lane, a
tile short of / equal to / one past a wave, three tiles) meet M = 1, 2, 64, 65, 127, 128 and 129 (one chunk short of / equal
to / one past 128, and the EM's own limit of 64 and one past it), alone and in a ragged batch with an image without lines
and one without VPs."""
import ctypes
import functools

import numpy as np
import pytest

import em_phase_reference as E
import estep_reference as R

pytestmark = pytest.mark.gpu

VPK_ERR_ARG = -1
MEASURE_ID = {"angle": 0, "dotprod": 1, "area": 2}
ALL = ("s", "lvsq", "p_lv", "p_l", "p_vl")


def _rt():
    from vanishing_points_2017_amd.runtime import get_runtime
    return get_runtime(0)


def _prob():
    from vanishing_points_2017_amd import probability_functions as prob
    return prob


def _dev(a, dtype=np.float64):
    rt = _rt()
    return rt.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(rt.tdev)


def run(images, measure, want=ALL):
    """vpk_estep_batch on a list of images (dicts of lp, l, v, s, p_v; host arrays): per image the outputs in the reference's
    shapes -- lvsq, p_lv (N, M), p_vl (M, N), p_l (N,), s (M,) -- as host arrays, None where not asked for."""
    prob, rt = _prob(), _rt()
    lo = prob._offsets_of([im["lp"].shape[0] for im in images])
    vo = prob._offsets_of([im["v"].shape[0] for im in images])

    def cat(key, width):
        return _dev(np.concatenate([np.asarray(im[key], dtype=np.float64).reshape((-1,) + width) for im in images]))

    with rt.on_stream():
        out = prob._estep(rt, lo, vo, cat("lp", (4,)), cat("l", (3,)), cat("v", (3,)), cat("s", ()), cat("p_v", ()),
                          MEASURE_ID[measure], want)
    rt.synchronize()
    host = {k: (None if x is None else x.cpu().numpy()) for k, x in out.items()}
    res, at = [], 0
    for b in range(len(images)):
        n, m = int(lo[b + 1] - lo[b]), int(vo[b + 1] - vo[b])
        o = {}
        for k in ("lvsq", "p_lv", "p_vl"):
            mat = None if host[k] is None else host[k][at:at + m * n].reshape(m, n)
            o[k] = mat if (mat is None or k == "p_vl") else mat.T.copy()
        o["p_l"] = None if host["p_l"] is None else host["p_l"][lo[b]:lo[b + 1]]
        o["s"] = None if host["s"] is None else host["s"][vo[b]:vo[b + 1]]
        res.append(o)
        at += m * n
    return res


@functools.lru_cache(maxsize=None)
def generated():
    """The generated cases and, per measure, their extended-precision references: computed once, shared, never changed."""
    cases = [R.case(n, m) for n, m in R.shapes()]
    refs = {meas: [R.reference(meas, c["v"], c["l"], c["lp"], c["s"], p_v=c["p_v"]) for c in cases] for meas in R.MEASURES}
    return cases, refs


def same(a, b, keys=R.KEYS + ("s",)):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("measure", R.MEASURES)
def test_every_golden_through_calc_probabilities(measure):
    """The whole call -- the prior by vpk_mixture_pdf, the E-step by vpk_estep_batch -- on every stored case with both
    variance vectors: within the bounds of the restatement, NaN where the reference has NaN, the caller's s left alone and
    the floored s what the reference wrote into it; calc_probabilities the numbers of calc_probabilities_batch."""
    prob = _prob()
    worst = {}
    for name in R.golden_names():
        g = R.golden(name)
        par = prob.PDFParams(means=g["means"], weights=g["weights"], sigma=float(g["sigma"]))
        for k in (0, 1):
            s = g["s_%s_%d" % (measure, k)]
            keep = s.copy()
            pdf = prob.calc_probabilities(0, par, g["v"][None], g["l"], g["lp"], s, None, distance_measure=measure)
            assert np.array_equal(s, keep)
            out = {"lvsq": pdf.lvsq, "p_lv": pdf.lv, "p_l": pdf.l, "p_vl": pdf.vl}
            ref = R.reference(measure, g["v"], g["l"], g["lp"], s, pdfpar=R.golden_pdfpar(g))
            what = "%s %s %d" % (name, measure, k)
            for key, x in R.check(out, ref, what).items():
                worst[key] = max(worst.get(key, 0.0), x)
            assert E._ratio(np.abs(R.ld(pdf.v) - ref["p_v"]), ref["b_p_v"]) <= 1.0, what
            for key in R.KEYS:
                assert np.array_equal(np.isnan(out[key]), np.isnan(g["out_%s_%d_%s" % (measure, k, key)])), (what, key)
            r = prob.calc_probabilities_batch(par, [g["v"]], [g["l"]], [g["lp"]], [s], distance_measure=measure)
            assert np.array_equal(r["s"][0].cpu().numpy(), g["out_%s_%d_s" % (measure, k)]), what
            one = r["pdf"][0]
            assert tuple(one.lvsq.shape) == pdf.lvsq.shape and tuple(one.vl.shape) == pdf.vl.shape
            for a, b in zip(one, pdf):
                assert np.array_equal(a.cpu().numpy(), b, equal_nan=True), what
    print("%s: worst error / bound %s" % (measure, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("measure", R.MEASURES)
def test_tile_edges_alone_and_in_a_ragged_batch(measure):
    """Every generated shape in one ragged launch, with an image without lines and one without VPs in it: within the
    bounds of the restatement; each image alone gives the bits it gives inside the batch; the launch that asks for lvsq
    and p_lv only, which splits the VP range over the grid, gives the bits of the full launch."""
    cases, refs = generated()
    mid = cases[len(cases) // 2]
    empty_n = dict(mid, lp=np.zeros((0, 4)), l=np.zeros((0, 3)))
    empty_m = dict(mid, v=np.zeros((0, 3)), s=np.zeros(0), p_v=np.zeros(0))
    images = cases[:3] + [empty_n] + cases[3:7] + [empty_m] + cases[7:]
    where = [i for i, im in enumerate(images) if im is not empty_n and im is not empty_m]
    batch = run(images, measure)
    split = run(images, measure, want=("lvsq", "p_lv"))
    only = run(images, measure, want=("lvsq",))
    worst = 0.0
    for c, ref, i in zip(cases, refs[measure], where):
        what = "%s N=%d M=%d" % (measure, c["lp"].shape[0], c["v"].shape[0])
        worst = max([worst] + list(R.check(batch[i], ref, what).values()))
        assert np.array_equal(batch[i]["s"], np.maximum(c["s"], 1e-200))
        assert same(split[i], batch[i], ("lvsq", "p_lv")) and same(only[i], batch[i], ("lvsq",)), what + ": the split launch differs"
        assert same(run([c], measure)[0], batch[i]), what + ": other bits alone than in the batch"
    print("%s: worst error / bound %.3g" % (measure, worst))
    assert batch[3]["lvsq"].size == 0 and batch[8]["p_l"].shape[0] == mid["lp"].shape[0]
    assert (batch[8]["p_l"] == 0).all(), "an image without VPs gets no workgroup: its p_l stays as allocated"


@pytest.mark.parametrize("n,m", [(1, 1), (7, 5), (64, 33), (65, 64), (129, 9), (257, 32)])
def test_angle_is_the_em_workgroups_estep_bit_for_bit(n, m):
    """lvsq equals kernels.estep's (the EM workgroup's own E-step); fed its p(v), p_l and p_vl do too."""
    from vanishing_points_2017_amd import kernels
    c = E.estep_case(n, m)
    pv, lvsq, pvl, pl, s = kernels.estep(c["lp"], c["cnn"], c["v"], c["s"])
    out = run([{"lp": c["lp"], "l": np.zeros((n, 3)), "v": c["v"], "s": c["s"], "p_v": pv}], "angle")[0]
    assert np.array_equal(out["s"], s)
    assert np.array_equal(out["lvsq"], lvsq, equal_nan=True)
    assert np.array_equal(out["p_l"], pl, equal_nan=True)
    assert np.array_equal(out["p_vl"], pvl, equal_nan=True)


def test_single_image_functions_are_the_batch_forms():
    prob = _prob()
    g = R.golden("yud_n65_m5")
    c = generated()[0][-1]                                   # N = 130, M = 129
    for v, l, lp in ((g["v"], g["l"], g["lp"]), (c["v"], c["l"], c["lp"])):
        for measure, fn in (("angle", prob.calc_lvsq_angle), ("dotprod", prob.calc_lvsq_dotprod), ("area", prob.calc_lvsq_area)):
            two = prob.calc_lvsq_batch([v, v[:1]], [l, l[:2]], [lp, lp[:2]], distance_measure=measure)
            assert tuple(two[0].shape) == (lp.shape[0], v.shape[0]) and tuple(two[1].shape) == (2, 1)
            got = fn(np.ascontiguousarray(v.T), l, lp, None)
            assert got.shape == (lp.shape[0], v.shape[0]) and np.array_equal(got, two[0].cpu().numpy(), equal_nan=True)
            assert np.array_equal(two[1].cpu().numpy(), got[:2, :1], equal_nan=True)
    ang = prob.calc_lvsq_angle(np.ascontiguousarray(g["v"].T), None, g["lp"], None)
    area = prob.calc_lvsq_area(np.ascontiguousarray(g["v"].T), None, g["lp"], None)
    for n, m in ((0, 0), (17, 3), (64, 4)):
        assert prob.calc_lvsq_single(g["v"][m], g["l"][n], g["lp"][n]) == ang[n, m]
        assert prob.calc_lvsq_area_single(g["v"][m], g["l"][n], g["lp"][n]) == area[n, m]
    with pytest.raises(ValueError):
        prob.calc_lvsq_batch([g["v"]], None, [g["lp"]], distance_measure="dotprod")


def test_bad_arguments_and_empty_calls():
    rt = _rt()
    t = rt.torch
    g = R.golden("yud_n65_m5")
    n, m = g["lp"].shape[0], g["v"].shape[0]
    with rt.on_stream():
        lp, l, v, s, pv = _dev(g["lp"]), _dev(g["l"]), _dev(g["v"]), _dev(g["s_angle_1"]), _dev(g["out_angle_1_p_v"])
        outs = [t.full((k,), -7.0, dtype=t.float64, device=rt.tdev) for k in (m, n * m, n * m, n, n * m)]
    rt.synchronize()
    P = rt.ptr
    lo, vo = np.array([0, n], np.int64), np.array([0, m], np.int64)

    def off(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(batch=1, lo=lo, vo=vo, lp=lp, l=l, v=v, s=s, pv=pv, measure=0, o=outs, h=rt.h):
        return rt.lib.vpk_estep_batch(h, batch, off(lo), off(vo), P(lp), P(l), P(v), P(s), P(pv), measure, *[P(x) for x in o])

    assert call(batch=-1) == VPK_ERR_ARG and call(h=None) == VPK_ERR_ARG
    assert call(measure=3) == VPK_ERR_ARG and call(measure=-1) == VPK_ERR_ARG
    assert call(lo=None) == VPK_ERR_ARG and call(vo=None) == VPK_ERR_ARG
    assert call(lo=np.array([n, 0], np.int64)) == VPK_ERR_ARG and call(vo=np.array([m, 0], np.int64)) == VPK_ERR_ARG
    assert call(lo=np.array([-1, n], np.int64)) == VPK_ERR_ARG
    assert call(lp=None) == VPK_ERR_ARG and call(v=None) == VPK_ERR_ARG and call(s=None) == VPK_ERR_ARG
    assert call(pv=None) == VPK_ERR_ARG, "p_l / p_vl asked for without p_v"
    assert call(l=None, measure=1) == VPK_ERR_ARG, "dotprod without the homogeneous lines"
    # empty calls do nothing, whatever the pointers
    assert call(batch=0) == 0 and call(batch=0, lo=None, vo=None, lp=None, v=None, s=None) == 0
    assert call(lo=np.array([0, 0], np.int64), lp=None) == 0 and call(vo=np.array([0, 0], np.int64), v=None, s=None) == 0
    assert call(o=[None] * 5, lp=None) == 0
    rt.synchronize()
    assert all((x.cpu().numpy() == -7.0).all() for x in outs)
    # l may be null for angle and area, p_v when neither p_l nor p_vl is asked for; every output may be null on its own
    assert call(l=None, measure=2) == 0
    assert call(pv=None, o=outs[:3] + [None, None]) == 0
    assert call(l=None) == 0
    rt.synchronize()
    full = [x.cpu().numpy().copy() for x in outs]
    assert not any((x == -7.0).any() for x in full)
    for k in range(5):
        o = [None] * 5
        o[k] = outs[k]
        with rt.on_stream():
            outs[k].fill_(-7.0)
        assert call(o=o) == 0
        rt.synchronize()
        assert np.array_equal(outs[k].cpu().numpy(), full[k], equal_nan=True), "output %d alone" % k


def test_two_calls_give_the_same_bits():
    cases, _ = generated()
    for measure in R.MEASURES:
        a, b = run(cases[-3:], measure), run(cases[-3:], measure)
        assert all(same(x, y) for x, y in zip(a, b))
