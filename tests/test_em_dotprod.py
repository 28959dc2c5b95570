"""distance_measure="dotprod" in the EM, without a GPU: the host build of the device source's em_run<MEASURE>
(tests/hostsim/sim_em_measure.cpp) against the recorded runs of the reference (tests/em_dotprod_cases.py), and the Python
surface's refusals.  The kernel itself: tests/test_gpu_em_dotprod.py."""
import numpy as np
import pytest

from em_dotprod_cases import case, check_last_estep, same_bits, stems
from golden_util import abserr, check_em_result, em_kwargs, load
from hostsim import simlib, simlib_measure


def _run(stem, **extra):
    g, kw, _ = case(stem)
    res = simlib_measure.em_single(g["l"].copy(), g["lp"], g["cnn_response"], g["sphere_image"], distance_measure="dotprod",
                                   want_distribution=True, **dict(kw, **extra))
    if res["status"] != 0:
        res["vp"] = None
    return res


_full = {}


def _unsliced(stem):
    if stem not in _full:
        _full[stem] = _run(stem)
    return _full[stem]


def test_the_recorded_cases_are_the_ones_asked_for():
    table = {"tiny_n12": (1, 2), "clean3_n60": (1, 3), "noweights_n100": (5, 9), "yud_n120": (17, 12), "nosplit_n150": (12, 9),
             "yud_n200": (6, 11), "mergeabort_n200": (16, 16), "periodicmerge_n220": (10, 12), "yud_n250": (25, 15),
             "ecd_n300_v8": (15, 19), "stress_n300__noinit": (49, 18), "stress_n1000__noinit": (49, 24),
             "stress_n300": (49, 7), "stress_n1000": (49, 8)}      # (the last two: with the stored init_vp)
    have = stems()
    for stem, (iters, m) in table.items():
        assert stem in have
        r = case(stem)[2]
        assert (int(r["o_iterations"]), r["o_vp"].shape[0]) == (iters, m), stem
    assert any("split_merge_freq" in case(s)[1] and case(s)[1]["split_merge_freq"] == 3 for s in have)
    assert any("init_vp" in case(s)[2] for s in have)
    assert max(case(s)[0]["lp"].shape[0] for s in have) >= 512      # mstep_lb<8>, the large pair pass, one thread per line


@pytest.mark.parametrize("stem", stems())
def test_host_build_meets_the_bar_on_every_recorded_case(stem):
    g, _, r = case(stem)
    res = _unsliced(stem)
    assert abserr(res["l"], g["l_normalised"]) <= 1e-15
    check_em_result(res, r)


@pytest.mark.parametrize("stem", stems())
def test_host_builds_last_estep_is_the_recorded_one(stem):
    """lvsq and p_vl of the last E-step (EM_result['distribution']) against the recorded arrays, within the tolerances worked
    out in em_dotprod_cases.check_last_estep."""
    res = _unsliced(stem)
    check_last_estep(res["vp"], res["sigma"], res["lvsq"], res["p_vl"], case(stem)[2])


@pytest.mark.parametrize("stem", [s for s in stems() if "n1000" not in s])
def test_a_run_suspended_at_every_checkpoint_gives_the_same_bits(stem):
    res = _run(stem, sliced=True)
    if int(case(stem)[2]["o_iterations"]) > 1:
        assert res["slices"] >= 1
    same_bits(res, _unsliced(stem))


@pytest.mark.parametrize("budget", [96, 2048])
def test_small_lds_budgets_take_the_chunked_smoother(budget):
    """yud_n120 (up to 25 hypotheses, 12 at the end) with a small LDS budget.  The host build has one lane, so smooth_plan can
    only answer 0 or 1 here (2 and 3 need a 64-lane wave: tests/test_gpu_em_dotprod.py runs those on the GPU): 96 doubles
    hold no operand panel at all (plan 0, smooth_blocks, a few rows per chunk); 2048 doubles hold the whole [line][Wp] panel
    while Wp <= 16 (plan 1) and give plan 0 with smooth_full in passes of 16 VPs beyond that.  Another summation order than
    the default budget's, so the bar is the reference's and not bit equality."""
    assert 120 * 8 > 96 and 120 * 16 <= 2048 < 120 * 24
    r = case("yud_n120")[2]
    res = _run("yud_n120", lds_doubles=budget)
    check_em_result(res, r)
    assert np.array_equal(res["vp_assoc"], _unsliced("yud_n120")["vp_assoc"])
    assert res["iterations"] == _unsliced("yud_n120")["iterations"]


@pytest.mark.parametrize("name", ["tiny_n12", "yud_n120", "stress_n300"])
def test_angle_through_the_template_is_the_untemplated_call(name):
    """em_run<VPK_DIST_ANGLE> of the new driver against sim_em.cpp's em_run(c, o, sl): templating moved nothing."""
    g = load(name)
    kw = em_kwargs(g)
    a = simlib_measure.em_single(g["l"].copy(), g["lp"], g["cnn_response"], g["sphere_image"], distance_measure="angle", **kw)
    b = simlib.em_single(g["l"].copy(), g["lp"], g["cnn_response"], g["sphere_image"], **kw)
    same_bits(a, b)
    assert np.array_equal(a["l"], b["l"])


def test_dotprod_is_another_result_than_angle():
    g, kw, _ = case("yud_n120")
    a = simlib.em_single(g["l"].copy(), g["lp"], g["cnn_response"], g["sphere_image"], **kw)
    assert a["iterations"] != _unsliced("yud_n120")["iterations"] or a["vp"].shape != _unsliced("yud_n120")["vp"].shape


@pytest.mark.parametrize("measure", ["area", "cosine", None, 1])
def test_other_measures_are_refused_before_the_gpu_is_touched(measure, monkeypatch):
    from vanishing_points_2017_amd import em as gem, vp_localisation

    def no_gpu(*a, **k):
        raise RuntimeError("the GPU was asked for")
    monkeypatch.setattr(gem, "get_runtime", no_gpu)
    g = load("tiny_n12")
    sc = {"l": g["l"].copy(), "lp": g["lp"], "cnn_response": g["cnn_response"], "sphere_image": g["sphere_image"]}
    with pytest.raises(AssertionError, match=repr(measure).replace("'", ".")):
        gem.em_batch([sc], distance_measure=measure)
    with pytest.raises(AssertionError):
        vp_localisation.expectation_maximisation_batch([sc["l"]], [sc["lp"]], [sc["cnn_response"]], [sc["sphere_image"]],
                                                       distance_measure=measure)


def test_the_single_image_drop_in_still_refuses_dotprod(monkeypatch):
    from vanishing_points_2017_amd import em as gem, vp_localisation

    def no_gpu(*a, **k):
        raise RuntimeError("the GPU was asked for")
    monkeypatch.setattr(gem, "get_runtime", no_gpu)
    g = load("tiny_n12")
    with pytest.raises(AssertionError):
        vp_localisation.expectation_maximisation(g["l"].copy(), g["lp"], g["cnn_response"], sphere_image=g["sphere_image"],
                                                 distance_measure="dotprod")


def test_the_setter_is_declared_and_exported():
    from vanishing_points_2017_amd import _lib, em as gem
    assert "vpk_em_set_distance_measure" in _lib.EXPORTS
    assert gem.EM_MEASURES == {"angle": 0, "dotprod": 1}
