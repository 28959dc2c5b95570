"""The E-step's three passes (csrc/em_estep.hpp: the exp and the division to p_vl only for the terms that do not underflow)
against the dense form vpk_em_set_smoother(h, 1) keeps, on the GPU: a pure speed choice, so every output agrees bit for bit.

The hand-made inputs are tests/estep_zeros_cases.py's (the host build's test, tests/test_em_estep_zeros.py, runs the same):
N = 12, 64, 65, 130, 257 give 8, 4, 2, 2 lanes per line and one lane per line with a ragged fifth wave.  vpk_estep plans with
6144 doubles and vpk_estep_smooth with the batch kernel's budget or the one vpk_em_set_lds_panel sets: at the default the
panel is the row-sliced one (plan 2) wherever M <= 32, at 4600 doubles -- below the row-sliced smoother's reduction scratch
alone, 4608 -- it is smooth_full's (plan 1) wherever N Wp fits; the plan each call took is asserted from info_out.  Both
entry points run "angle"; "dotprod" runs in the whole EM below, on the recorded cases of tests/golden/em_dotprod/."""
import numpy as np
import pytest

import em_dotprod_cases as dp
import estep_zeros_cases as zc
from conftest import golden_cases
from golden_util import em_kwargs, gpu_rasters, load

pytestmark = pytest.mark.gpu

OUTPUTS = ("vp", "sigma", "counts", "counts_weighted", "num_vp", "vp_assoc", "iterations", "status", "flags")
PLAN1_BUDGET = 4600
SMALL_BUDGET = 8192        # whole EM: images up to ~140 lines keep the row-sliced panel, the larger ones take smooth_full's


def _modes(fn):
    """fn() under the default and under vpk_em_set_smoother(h, 1)"""
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    new = fn()
    rt.handle.em_set_smoother(1)
    try:
        old = fn()
    finally:
        rt.handle.em_set_smoother(0)
    return new, old


def _estep(c):
    from vanishing_points_2017_amd import kernels
    pv, lvsq, pvl, pl, s = kernels.estep(c["lp"], c["cnn"], c["v"], c["s"])
    return {"p_v": pv, "lvsq": lvsq, "p_vl": pvl, "p_l": pl, "s": s}


def _estep_smooth(c):
    from vanishing_points_2017_amd import kernels
    pvl, w, s, info = kernels.estep_smooth(c["lp"], c["cnn"], c["v"], c["s"], c["lweight"], c["lsim"])
    return {"p_vl": pvl, "w": w, "s": s, "info": info}


@pytest.mark.parametrize("n", zc.SHAPES_N)
def test_edge_inputs_through_the_entry_points(n):
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    plans = set()
    for m in zc.SHAPES_M:
        for variant in zc.VARIANTS:
            c = zc.case(n, m, variant)
            new, old = _modes(lambda: _estep(c))
            zc.same_bits(new, old, ("p_v", "lvsq", "p_vl", "p_l", "s"))
            for budget in (0, PLAN1_BUDGET):
                rt.handle.em_set_lds_panel(budget)
                try:
                    new, old = _modes(lambda: _estep_smooth(c))
                finally:
                    rt.handle.em_set_lds_panel(0)
                label = (n, m, variant, budget)
                zc.same_bits(new, old, ("p_vl", "w", "s"))
                plan = int(new["info"][0])
                if m > 32:                                   # (setting 1 plans no row-sliced panel: its info_out differs)
                    assert plan in (0, 3), label
                elif budget == 0:
                    assert plan == 2 and int(new["info"][1]) == 0x100 + 8 * ((m + 7) // 8), label
                elif n * 8 * ((m + 7) // 8) <= PLAN1_BUDGET:
                    assert plan == 1 and int(new["info"][1]) == 8 * ((m + 7) // 8), label
                plans.add(plan)
    assert {1, 2} <= plans


# ---- whole EM ----------------------------------------------------------------------------------------------------------------
def _host(out):
    return {k: out[k].cpu().numpy() for k in OUTPUTS}


def _run(rt, scenes, mode, budget=0, measure="angle", **kw):
    from vanishing_points_2017_amd import em as gem
    d = gem.upload_batch(rt, [dict(s, l=s["l"].copy()) for s in scenes])
    rt.handle.em_set_smoother(mode)
    rt.handle.em_set_lds_panel(budget)
    try:
        out = gem.em_batch_device(rt, d["offsets"], d["l"], d["lp"], d["cnn"], d["sphere"], d["init_vp"], gem._params(kw),
                                  distance_measure=measure)
        rt.synchronize()
    finally:
        rt.handle.em_set_smoother(0)
        rt.handle.em_set_lds_panel(0)
    return _host(out)


def _assert_same(got, want):
    for k in OUTPUTS:
        assert np.array_equal(got[k], want[k], equal_nan=True), k


@pytest.fixture(scope="module")
def scenes24():
    from vanishing_points_2017_amd import synth
    return gpu_rasters(synth.config_scenes(2, count=24))


@pytest.mark.parametrize("budget", [0, SMALL_BUDGET])
def test_scenes_default_against_the_dense_form(scenes24, budget):
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    want = _run(rt, scenes24, 1, budget)
    assert (want["status"] == 0).all() and want["iterations"].max() > 10
    _assert_same(_run(rt, scenes24, 0, budget), want)


@pytest.mark.parametrize("budget", [0, SMALL_BUDGET])
def test_goldens_default_against_the_dense_form(budget):
    """every stored case in one launch per keyword set would mix keywords: one launch per case, all in one test"""
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    for name in golden_cases():
        g = load(name)
        kw = em_kwargs(g)
        sc = {"l": g["l"], "lp": g["lp"], "cnn_response": g["cnn_response"], "sphere_image": g["sphere_image"],
              "init_vp": kw.pop("init_vp", None)}
        want = _run(rt, [sc], 1, budget, **kw)
        assert int(want["status"][0]) == int(g["o_status"]), name
        _assert_same(_run(rt, [sc], 0, budget, **kw), want)


@pytest.mark.parametrize("budget", [0, SMALL_BUDGET])
def test_dotprod_goldens_default_against_the_dense_form(budget):
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    for stem in dp.stems():
        sc, kw = dp.scene(stem)
        want = _run(rt, [sc], 1, budget, "dotprod", **kw)
        assert int(want["iterations"][0]) == int(dp.case(stem)[2]["o_iterations"]), stem
        _assert_same(_run(rt, [sc], 0, budget, "dotprod", **kw), want)


def test_time_sliced_default_against_the_uninterrupted_dense_form(scenes24):
    """a slice shorter than the set-up, eight launches in flight before the flush (tests/test_gpu_em_split_events.py): images
    are parked between an E-step and the smoother's next call many times, and resumed by other launches"""
    from vanishing_points_2017_amd import em as gem
    from vanishing_points_2017_amd.runtime import get_runtime
    want = _run(get_runtime(0), scenes24, 1)
    rt = get_runtime(0, "estep_zeros_slice")
    d = gem.upload_batch(rt, [dict(s, l=s["l"].copy()) for s in scenes24])
    rt.handle.em_set_time_slice(0.3, int(np.diff(d["offsets"]).max()))
    outs, lines = [], []           # (a launch's lines are normalised in place, by whichever launch starts the image: kept alive)
    try:
        for _ in range(8):
            lines.append(d["l"].clone())
            outs.append(gem.em_batch_device(rt, d["offsets"], lines[-1], d["lp"], d["cnn"], d["sphere"], d["init_vp"],
                                            gem._params({})))
        with rt.on_stream():
            rt.handle.em_flush()
        rt.synchronize()
    finally:
        rt.handle.em_set_time_slice(0.0)
    for out in outs:
        _assert_same(_host(out), want)
