"""The E-step's call surface without a GPU: the extended-precision restatement (tests/estep_reference.py) against the
reference's stored output (tests/golden/estep/), the device code (csrc/estep_device.hpp) compiled for the host by
tests/hostsim/sim_estep.cpp and run serially against both, and the host side of probability_functions.  The kernel itself:
tests/test_gpu_estep_surface.py."""
import ctypes
import os

import numpy as np
import pytest

import em_phase_reference as E
import estep_reference as R
from hostsim import hostbuild

MEASURE_ID = {"angle": 0, "dotprod": 1, "area": 2}


@pytest.fixture(scope="module")
def sim():
    lib = hostbuild.load("estep")
    D, L, I = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong), ctypes.c_int
    lib.sim_estep_batch.argtypes = [I, L, L, D, D, D, D, D, I, I, D, D, D, D, D]
    return lib


def _d(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None


def run_sim(sim, images, measure, want=("s", "lvsq", "p_lv", "p_l", "p_vl"), split=-1):
    """sim_estep_batch on a list of images (dicts of lp, l, v, s, p_v): per image a dict of the outputs in the reference's
    shapes -- lvsq, p_lv (N, M), p_vl (M, N), p_l (N,), s (M,).  Outputs are pre-filled with -7."""
    lo = np.concatenate(([0], np.cumsum([im["lp"].shape[0] for im in images]))).astype(np.int64)
    vo = np.concatenate(([0], np.cumsum([im["v"].shape[0] for im in images]))).astype(np.int64)

    def cat(key, width):
        return np.ascontiguousarray(np.concatenate([np.asarray(im[key], dtype=np.float64).reshape((-1,) + width) for im in images]))

    lp, l, v, s, pv = cat("lp", (4,)), cat("l", (3,)), cat("v", (3,)), cat("s", ()), cat("p_v", ())
    total = int((np.diff(lo) * np.diff(vo)).sum())
    size = {"s": int(vo[-1]), "lvsq": total, "p_lv": total, "p_l": int(lo[-1]), "p_vl": total}
    buf = {k: (np.full(size[k], -7.0) if k in want else None) for k in size}
    keep = s.copy()
    L = ctypes.POINTER(ctypes.c_longlong)
    rc = sim.sim_estep_batch(len(images), lo.ctypes.data_as(L), vo.ctypes.data_as(L), _d(lp), _d(l), _d(v), _d(s), _d(pv),
                             MEASURE_ID[measure], split, _d(buf["s"]), _d(buf["lvsq"]), _d(buf["p_lv"]), _d(buf["p_l"]),
                             _d(buf["p_vl"]))
    assert rc == 0
    assert np.array_equal(s, keep, equal_nan=True), "the caller's s was written"
    out, at = [], 0
    for b in range(len(images)):
        n, m = int(lo[b + 1] - lo[b]), int(vo[b + 1] - vo[b])
        o = {}
        for k in ("lvsq", "p_lv", "p_vl"):
            o[k] = None if buf[k] is None else (buf[k][at:at + m * n].reshape(m, n) if k == "p_vl" else buf[k][at:at + m * n].reshape(m, n).T.copy())
        o["p_l"] = None if buf["p_l"] is None else buf["p_l"][lo[b]:lo[b + 1]]
        o["s"] = None if buf["s"] is None else buf["s"][vo[b]:vo[b + 1]]
        out.append(o)
        at += m * n
    return out


def golden_runs():
    for name in R.golden_names():
        g = R.golden(name)
        for meas in R.MEASURES:
            for k in (0, 1):
                yield name, g, meas, k


def recorded(g, meas, k):
    return {f: g["out_%s_%d_%s" % (meas, k, f)] for f in ("p_v", "angles", "lvsq", "p_lv", "p_l", "p_vl", "s")}


def test_goldens_are_small_and_complete():
    names = R.golden_names()
    assert len(names) == 4
    size = sum(os.path.getsize(os.path.join(R.GOLDEN, n + ".npz")) for n in names)
    assert size < 500000
    shapes = {tuple(R.golden(n)["lp"].shape[:1]) + tuple(R.golden(n)["v"].shape[:1]) for n in names}
    assert (1, 1) in shapes and all(n <= 65 and m <= 5 for n, m in shapes)
    g = R.golden("clean3_n60_m4_infinite_vp")
    assert g["v"][3, 2] == 0
    for meas in ("angle", "area"):
        assert np.isnan(g["out_%s_0_lvsq" % meas][:, 3]).all() and not np.isnan(g["out_%s_0_lvsq" % meas][:, :3]).any()
    assert np.isfinite(g["out_dotprod_1_lvsq"]).all() and np.isfinite(g["out_dotprod_1_p_vl"]).all()
    g = R.golden("tiny_n12_m2_zero_s_mixture130")
    assert g["s_angle_0"][0] == 0 and g["out_angle_0_s"][0] == 1e-200 and g["weights"].shape == (130,)


def test_no_committed_area_element_is_without_a_bound():
    worst = np.inf
    for name in R.golden_names():
        g = R.golden(name)
        lvsq, bound, rel = R.lvsq_area(g["v"], g["lp"])
        fin = ~np.isnan(lvsq.astype(np.float64))
        assert np.isfinite(bound[fin]).all(), name
        if fin.any():
            worst = min(worst, float(rel[fin].min()))
    print("smallest relative radicand of a committed case: %.3g" % worst)
    assert worst >= float(R.MIN_REL_RADICAND)
    gen, count = np.inf, 0
    for n, m in R.shapes():                                  # the generated cases of both test files likewise
        c = R.case(n, m)
        lvsq, bound, rel = R.lvsq_area(c["v"], c["lp"])
        fin = ~np.isnan(lvsq.astype(np.float64))
        assert fin.all() and np.isfinite(bound).all(), (n, m)
        gen, count = min(gen, float(rel.min())), count + rel.size
    print("smallest relative radicand of a generated case: %.3g (%d elements)" % (gen, count))
    assert gen >= float(R.MIN_REL_RADICAND)


def test_restatement_meets_every_golden():
    """The reference's recorded values lie inside the bounds around the extended-precision restatement: NumPy's own
    roundings (np.dot's BLAS order for dotprod and p_l among them) are operations of the kind the bounds count."""
    worst = {}
    for name, g, meas, k in golden_runs():
        ref = R.reference(meas, g["v"], g["l"], g["lp"], g["s_%s_%d" % (meas, k)], pdfpar=R.golden_pdfpar(g))
        rec = recorded(g, meas, k)
        assert np.array_equal(rec["s"], ref["s"].astype(np.float64))
        w = R.check(rec, ref, "%s %s %d" % (name, meas, k))
        r = E._ratio(np.abs(R.ld(rec["p_v"]) - ref["p_v"]), ref["b_p_v"])
        assert r <= 1.0
        for key, x in w.items():
            worst[(meas, key)] = max(worst.get((meas, key), 0.0), x)
    for meas in R.MEASURES:
        print("%-8s recorded NumPy values, worst error / bound: %s" % (
            meas, ", ".join("%s %.3g" % (key, worst[(meas, key)]) for key in R.KEYS)))
    # the second variance vector does its work: most lines are off the 1e-12 floor
    g = R.golden("yud_n65_m5")
    assert (g["out_dotprod_0_p_l"] == 1e-12).sum() > 40 and (g["out_dotprod_1_p_l"] == 1e-12).sum() < 10


def test_probabilities_scheme_is_em_phase_references():
    """R.probabilities on the angle measure's lvsq returns what em_phase_reference.estep_reference returns."""
    g = R.golden("yud_n65_m5")
    par = R.golden_pdfpar(g)
    for s in (g["s_angle_0"], g["s_angle_1"]):
        a = E.estep_reference(par, g["v"], g["lp"], s)
        b = R.reference("angle", g["v"], g["l"], g["lp"], s, pdfpar=par)
        for ka, kb in (("lvsq", "lvsq"), ("b_lvsq", "b_lvsq"), ("p_lv", "p_lv"), ("p_l", "p_l"), ("b_pl", "b_p_l"), ("p_vl", "p_vl"),
                       ("b_pvl", "b_p_vl"), ("s", "s")):
            assert np.array_equal(a[ka], b[kb], equal_nan=True), ka


def test_host_build_meets_every_golden(sim):
    worst = {}
    for name, g, meas, k in golden_runs():
        rec = recorded(g, meas, k)
        im = {"lp": g["lp"], "l": g["l"], "v": g["v"], "s": g["s_%s_%d" % (meas, k)], "p_v": rec["p_v"]}
        out = run_sim(sim, [im], meas)[0]
        assert np.array_equal(out["s"], rec["s"]), "s floored at 1e-200"
        ref = R.reference(meas, g["v"], g["l"], g["lp"], im["s"], pdfpar=R.golden_pdfpar(g))
        for key, x in R.check(out, ref, "%s %s %d" % (name, meas, k)).items():
            worst[(meas, key)] = max(worst.get((meas, key), 0.0), x)
        for key in R.KEYS:                                   # and the NaN positions are the reference's own
            assert np.array_equal(np.isnan(out[key]), np.isnan(rec[key])), (name, meas, key)
    for meas in R.MEASURES:
        print("%-8s host build, worst error / bound: %s" % (meas, ", ".join("%s %.3g" % (key, worst[(meas, key)]) for key in R.KEYS)))


@pytest.mark.parametrize("measure", R.MEASURES)
def test_host_build_at_the_tile_edges(sim, measure):
    """The generated shapes against the restatement; the launch split over the VP range, an image alone and an image in a
    ragged batch (with one image without lines and one without VPs) give the same bits."""
    cases = [R.case(n, m) for n, m in R.shapes()]
    worst = 0.0
    for c in cases:
        out = run_sim(sim, [c], measure)[0]
        ref = R.reference(measure, c["v"], c["l"], c["lp"], c["s"], p_v=c["p_v"])
        worst = max([worst] + list(R.check(out, ref, "%s N=%d M=%d" % (measure, c["lp"].shape[0], c["v"].shape[0])).values()))
        part = run_sim(sim, [c], measure, want=("lvsq", "p_lv"))[0]
        assert np.array_equal(part["lvsq"], out["lvsq"], equal_nan=True) and np.array_equal(part["p_lv"], out["p_lv"], equal_nan=True)
    print("%s: worst error / bound %.3g" % (measure, worst))
    pick = [cases[0], cases[-1], cases[len(cases) // 2]]
    empty_n = dict(pick[1], lp=np.zeros((0, 4)), l=np.zeros((0, 3)))
    empty_m = dict(pick[1], v=np.zeros((0, 3)), s=np.zeros(0), p_v=np.zeros(0))
    batch = run_sim(sim, [pick[0], empty_n, pick[1], empty_m, pick[2]], measure)
    for b, c in ((0, pick[0]), (2, pick[1]), (4, pick[2])):
        alone = run_sim(sim, [c], measure)[0]
        for key in R.KEYS + ("s",):
            assert np.array_equal(batch[b][key], alone[key], equal_nan=True), key
    assert batch[1]["s"].tolist() == [-7.0] * pick[1]["v"].shape[0] and (batch[3]["p_l"] == -7.0).all()


@pytest.mark.parametrize("n,m", [(1, 1), (7, 5), (64, 33), (65, 64), (129, 9)])
def test_host_build_angle_is_the_em_workgroups_estep(sim, n, m):
    """The restated per-pair expression against the EM workgroup's own E-step (simlib.estep: em_device.hpp's estep on the
    host), bit for bit, fed its p(v)."""
    from hostsim import simlib
    c = E.estep_case(n, m)
    pv, lvsq, pvl, s = simlib.estep(c["lp"], c["cnn"], c["v"], c["s"])
    im = {"lp": c["lp"], "l": np.zeros((n, 3)), "v": c["v"], "s": c["s"], "p_v": pv}
    out = run_sim(sim, [im], "angle")[0]
    assert np.array_equal(out["s"], s)
    assert np.array_equal(out["lvsq"], lvsq.T, equal_nan=True)
    assert np.array_equal(out["p_vl"], pvl, equal_nan=True)


def test_python_surface_without_a_gpu():
    """What the module decides before it touches the GPU, and the two NumPy mirrors against the stored output."""
    from vanishing_points_2017_amd import probability_functions as prob
    g = R.golden("yud_n65_m5")
    for fn, args in ((prob.calc_lvsq_batch, ([g["v"]], [g["l"]], [g["lp"]])),
                     (prob.calc_probabilities_batch, (np.zeros((1, 20, 20), np.float32), [g["v"]], [g["l"]], [g["lp"]], [g["s_angle_0"]]))):
        for bad in ("euclid", None, 3):
            with pytest.raises(ValueError):
                fn(*args, distance_measure=bad)
    with pytest.raises(ValueError):
        prob.calc_probabilities(0, prob.PDFParams(g["means"], g["weights"], float(g["sigma"])), g["v"][None], g["l"], g["lp"],
                                g["s_angle_0"], None, distance_measure="triangle")
    for name, g, meas, k in golden_runs():
        rec = recorded(g, meas, k)
        s = g["s_%s_%d" % (meas, k)].copy()
        m, n = g["v"].shape[0], g["lp"].shape[0]
        assert np.array_equal(prob.calc_plv(m, g["v"].T, s, rec["lvsq"], g["lp"]), rec["p_lv"], equal_nan=True)
        assert np.array_equal(s, g["s_%s_%d" % (meas, k)]), "calc_plv wrote the caller's s"
        assert np.array_equal(prob.calc_pvl(m, n, rec["p_lv"], rec["p_v"], rec["p_l"]), rec["p_vl"], equal_nan=True)
    doc = prob.__doc__
    assert "calc_point" in doc and "calc_vp_line_triangles" in doc and "ValueError" in doc
