"""distance_measure="dotprod" in the persistent EM kernel (vpk_em_set_distance_measure, em.em_batch and the Python surface
above it) against the recorded runs of the reference (tests/em_dotprod_cases.py).  CPU twin: tests/test_em_dotprod.py."""
import numpy as np
import pytest

import estep_reference as R
import em_smoother_reference as S
from em_dotprod_cases import case, check_last_estep, same_bits, scene, stems
from golden_util import abserr, check_em_result

pytestmark = pytest.mark.gpu

_single = {}


def _one(stem):
    """The case alone in its launch, with the decision metric and the last E-step's distribution; computed once."""
    from vanishing_points_2017_amd import em as gem
    if stem not in _single:
        sc, kw = scene(stem)
        _single[stem] = gem.em_batch([sc], want_metric=True, want_distribution=True, distance_measure="dotprod", **kw)[0]
    return _single[stem]


def _groups():
    """The cases that one launch can take together: equal keywords, and init_vp of one shape or none."""
    out = {}
    for stem in stems():
        sc, kw = scene(stem)
        key = (tuple(sorted(kw.items())), None if sc["init_vp"] is None else sc["init_vp"].shape)
        out.setdefault(key, []).append(stem)
    return sorted(out.values(), key=len, reverse=True)


@pytest.mark.parametrize("stem", stems())
def test_every_recorded_case_meets_the_bar(stem):
    g, _, r = case(stem)
    res = _one(stem)
    assert res["status"] == 0 and res["flags"] & 4 == 0
    assert abserr(res["l"], g["l_normalised"]) <= 1e-15
    check_em_result(res, r)


@pytest.mark.parametrize("group", _groups(), ids=lambda g: g[0])
def test_one_ragged_launch_equals_the_single_runs(group):
    """Every case of a keyword set in ONE launch, an image without lines between them: the bits of the single runs."""
    from vanishing_points_2017_amd import em as gem
    scenes = [scene(s)[0] for s in group]
    kw = scene(group[0])[1]
    empty = dict(scenes[0], l=np.zeros((0, 3)), lp=np.zeros((0, 4)))
    scenes.insert(1, empty)
    res = gem.em_batch(scenes, want_metric=True, distance_measure="dotprod", **kw)
    assert res[1]["vp"] is None
    for stem, r in zip(group, res[:1] + res[2:]):
        same_bits(r, _one(stem), keys=("vp", "sigma", "counts", "counts_weighted", "vp_assoc", "decision_metric", "l"))


@pytest.mark.parametrize("stem", stems())
def test_last_estep_is_the_surface_kernels_and_the_recorded_one(stem):
    """EM_result['distribution'].lvsq is calc_lvsq_batch(..., "dotprod") on the result's VPs and normalised lines bit for bit
    (em_estep.hpp restates estep_device.hpp's expression operand for operand) and within estep_reference's rounding bound of
    the extended-precision value there; lvsq and p_vl agree with the arrays recorded from the reference within the
    tolerances worked out in em_dotprod_cases.check_last_estep (VPs to 1e-9, variances to 1e-9 relative, and what those
    two allow downstream)."""
    from vanishing_points_2017_amd import probability_functions as P
    g, _, r = case(stem)
    res = _one(stem)
    d = res["distribution"]
    surf = P.calc_lvsq_batch([res["vp"]], [res["l"]], [g["lp"]], "dotprod")[0].cpu().numpy()
    assert np.array_equal(d.lvsq, surf)
    ours, b_ours = R.lvsq_dotprod(res["vp"], res["l"])
    assert np.all(np.abs(R.ld(d.lvsq) - ours) <= b_ours)
    worst = check_last_estep(res["vp"], res["sigma"], d.lvsq, d.vl, r)
    print("%s: worst error / tolerance against the recording: lvsq %.2g, p_vl %.2g" % ((stem,) + worst))


# (case, LDS budget in doubles, the plan smooth_plan gives at the case's final VP count)
BUDGETS = [("yud_n120", 96, 0), ("yud_n120", 2048, 1), ("ecd_n300_v8", 96, 0), ("ecd_n300_v8", 7100, 3)]


@pytest.mark.parametrize("stem,budget,plan", BUDGETS)
def test_small_lds_budgets_take_the_chunked_plans(stem, budget, plan):
    """vpk_em_set_lds_panel under "dotprod": smooth_plan 0 (no operand panel: smooth_blocks / smooth_full in passes), 1 and 3
    (the E-step's weights go to HBM, smooth_rows in passes of rs_wfit VPs).  Plan 3 needs N Wp above the budget and the
    eight-VP sliced panel below it, which no budget gives an image of 120 lines with at most 32 hypotheses (asserted): the
    300-line case takes it, at 7100 doubles for every VP count from 17 to 32.  The default budget is plan 2 (every other
    test here).  The chunked plans sum in another order, so the bar is the reference's -- check_em_result, with it equal
    assignments and iterations -- and not bit equality."""
    from vanishing_points_2017_amd import em as gem
    from vanishing_points_2017_amd.runtime import get_runtime
    g, _, r = case(stem)
    n, m = g["lp"].shape[0], r["o_vp"].shape[0]
    assert S.smooth_plan(n, m, budget, 0) == plan and S.smooth_plan(n, m, S.DEFAULT_BUDGET, 0) == 2
    if stem == "yud_n120":
        assert not any(S.smooth_plan(n, k, wt, 0) == 3 for k in range(1, 33) for wt in range(64, S.DEFAULT_BUDGET + 8, 8))
    if plan == 3:
        assert all(S.smooth_plan(n, k, budget, 0) == 3 for k in range(17, 33))
    sc, kw = scene(stem)
    rt = get_runtime(0)
    rt.handle.em_set_lds_panel(budget)
    try:
        res = gem.em_batch([sc], distance_measure="dotprod", **kw)[0]
    finally:
        rt.handle.em_set_lds_panel(0)
    check_em_result(res, r)
    assert np.array_equal(res["vp_assoc"], _one(stem)["vp_assoc"]) and res["iterations"] == _one(stem)["iterations"]


def test_time_sliced_launches_give_the_same_bits_and_hold_the_measure():
    """vpk_em_set_time_slice under "dotprod": images suspended at a launch's deadline are resumed by later launches and the
    flush with the bits of uninterrupted runs; while images are parked the measure cannot be changed (VPK_ERR_STATE)."""
    from vanishing_points_2017_amd import _lib, em as gem
    from vanishing_points_2017_amd.runtime import get_runtime
    group = _groups()[0]
    assert len(group) >= 4
    rt = get_runtime(0, "dotprod_slice")
    scenes = [scene(s)[0] for s in group]
    p = gem._params(scene(group[0])[1])
    d = gem.upload_batch(rt, scenes)
    l0 = d["l"].clone()
    rt.handle.em_set_distance_measure(1)
    try:
        ref = gem.em_batch_device(rt, d["offsets"], l0.clone(), d["lp"], d["cnn"], d["sphere"], None, p,
                                  distance_measure="dotprod")
        rt.synchronize()
        ref = {k: v.cpu().numpy() for k, v in ref.items() if v is not None}
        assert ref["iterations"].max() >= 15
        rt.handle.em_set_time_slice(0.05, int(np.diff(d["offsets"]).max()))
        keep = []
        for _ in range(3):
            lb = l0.clone()
            keep.append((lb, gem.em_batch_device(rt, d["offsets"], lb, d["lp"], d["cnn"], d["sphere"], None, p,
                                                 distance_measure="dotprod")))
        with pytest.raises(_lib.VpkError, match="parked"):
            rt.handle.em_set_distance_measure(0)
        assert rt.handle.em_distance_measure == 1
        with rt.on_stream():
            rt.handle.em_flush()
        rt.synchronize()
        for lb, out in keep:
            got = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
            for k in ("status", "iterations", "num_vp", "vp_assoc", "flags"):
                assert np.array_equal(got[k], ref[k]), k
            for b in range(len(scenes)):
                m = int(ref["num_vp"][b])
                for k in ("vp", "sigma", "counts", "counts_weighted"):
                    assert np.array_equal(got[k][b, :m], ref[k][b, :m]), (k, b)
        for b, stem in enumerate(group):                      # ... which are the default lane's single runs
            m = int(ref["num_vp"][b])
            assert np.array_equal(ref["vp"][b, :m], _one(stem)["vp"])
    finally:
        rt.handle.em_set_time_slice(0.0)
        rt.handle.em_set_distance_measure(0)


def test_a_time_sliced_handle_at_another_measure_is_refused_before_the_launch():
    from vanishing_points_2017_amd import _lib, em as gem
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0, "dotprod_slice_guard")
    sc, kw = scene("tiny_n12")
    d = gem.upload_batch(rt, [sc])
    rt.handle.em_set_time_slice(0.05, 12)
    try:
        with pytest.raises(_lib.VpkError, match="time-sliced"):
            gem.em_batch_device(rt, d["offsets"], d["l"], d["lp"], d["cnn"], d["sphere"], None, gem._params(kw),
                                distance_measure="dotprod")
        assert rt.handle.em_distance_measure == 0
    finally:
        rt.handle.em_set_time_slice(0.0)


def test_setter_takes_the_two_measures_only():
    from vanishing_points_2017_amd import _lib
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0, "dotprod_setter")
    for bad in (2, 3, -1):                                    # VPK_DIST_AREA and anything else
        with pytest.raises(_lib.VpkError):
            rt.handle.em_set_distance_measure(bad)
        assert rt.handle.em_distance_measure == 0
    rt.handle.em_set_distance_measure(1)
    rt.handle.em_set_distance_measure(0)


def test_an_angle_run_after_a_dotprod_run_is_the_one_before_it():
    from vanishing_points_2017_amd import em as gem
    sc, kw = scene("yud_n120")
    before = gem.em_batch([dict(sc, l=sc["l"].copy())], want_metric=True, **kw)[0]
    dot = gem.em_batch([dict(sc, l=sc["l"].copy())], want_metric=True, distance_measure="dotprod", **kw)[0]
    after = gem.em_batch([dict(sc, l=sc["l"].copy())], want_metric=True, **kw)[0]
    keys = ("vp", "sigma", "counts", "counts_weighted", "vp_assoc", "decision_metric")
    same_bits(after, before, keys=keys)
    same_bits(dot, _one("yud_n120"), keys=keys)
    assert dot["iterations"] != before["iterations"] or dot["vp"].shape != before["vp"].shape
    check_em_result(before, case("yud_n120")[0])


def test_run_em_single_and_the_batch_twin_give_em_batchs_result():
    from vanishing_points_2017_amd import evaluation, vp_localisation
    keys = ("vp", "sigma", "counts", "counts_weighted", "vp_assoc", "decision_metric")
    g, kw, _ = case("yud_n120")
    assert not kw
    l = g["l"].copy()
    datum = {"lines": {"lines": l, "line_segments": g["lp"].copy()}, "cnn_prediction": g["cnn_response"].reshape(20, 20),
             "sphere_image": g["sphere_image"]}
    out = evaluation.run_em_single(datum, distance_measure="dotprod")
    res = dict(out["EM_result"], status=0)
    same_bits(res, _one("yud_n120"), keys=keys)
    assert np.array_equal(l, _one("yud_n120")["l"])           # normalised in place
    assert np.array_equal(res["distribution"].lvsq, _one("yud_n120")["distribution"].lvsq)
    # the batch twin: two cases of different keyword-free shapes in one call, and a keyword case with init_vp
    stems2 = ["yud_n120", "tiny_n12"]
    ls = [case(s)[0]["l"].copy() for s in stems2]
    res2 = vp_localisation.expectation_maximisation_batch(ls, [case(s)[0]["lp"] for s in stems2],
                                                          [case(s)[0]["cnn_response"] for s in stems2],
                                                          [case(s)[0]["sphere_image"] for s in stems2],
                                                          distance_measure="dotprod")
    for s, l_, r in zip(stems2, ls, res2):
        assert "status" not in r and "l" not in r
        same_bits(dict(r, status=0), _one(s), keys=keys)
        assert np.array_equal(l_, _one(s)["l"])
        assert np.array_equal(r["distribution"].vl, _one(s)["distribution"].vl)
    sc, kw = scene("yud_n120__initvp")
    r = vp_localisation.expectation_maximisation_batch([sc["l"]], [sc["lp"]], [sc["cnn_response"]], [sc["sphere_image"]],
                                                       init_vps=[sc["init_vp"]], distance_measure="dotprod", **kw)[0]
    same_bits(dict(r, status=0), _one("yud_n120__initvp"), keys=keys)
    angle = vp_localisation.expectation_maximisation_batch([case("yud_n120")[0]["l"].copy()], [g["lp"]], [g["cnn_response"]],
                                                           [g["sphere_image"]])[0]
    check_em_result(angle, g)
