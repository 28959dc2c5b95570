"""The E-step's three passes (csrc/em_estep.hpp: the exp and the division to p_vl only for the terms that do not underflow)
against the dense form that EmCtx::smoother = 1 keeps, in the host build of the device source: every output of the E-step
and the weight panel as the smoother reads it, bit for bit.  The host build has one lane, so this is the one-lane-per-line
form over smooth_full's panel (plan 1); the forms with several lanes per line and the row-sliced panel are the GPU tests'
(tests/test_gpu_em_estep_zeros.py, same inputs)."""
import numpy as np
import pytest

import em_dotprod_cases as dp
import estep_zeros_cases as zc
from conftest import golden_cases
from golden_util import em_kwargs, load
from hostsim import simlib_estep_zeros as sim

BUDGET = 18800            # doubles of LDS the phases plan with: what a CU leaves the batch kernel (include/vpk.h)
ESTEP_OUT = ("p_v", "lvsq", "p_vl", "w", "s")
EM_OUT = ("vp", "sigma", "counts", "counts_weighted", "vp_assoc", "lvsq", "p_vl")


def _both(c, measure):
    return [sim.estep_smooth(c["l"], c["lp"], c["cnn"], c["v"], c["s"], c["lweight"], c["lsim"], measure=measure,
                             smoother=mode, lds_doubles=BUDGET) for mode in (0, 1)]


@pytest.mark.parametrize("measure", ["angle", "dotprod"])
@pytest.mark.parametrize("n", zc.SHAPES_N)
def test_three_passes_give_the_dense_forms_bits(n, measure):
    seen = set()
    for m in zc.SHAPES_M:
        for variant in zc.VARIANTS:
            c = zc.case(n, m, variant)
            new, old = _both(c, measure)
            label = (n, m, variant, measure)
            assert new["plan"] == (1 if m <= 32 else 0), label         # M <= 32: the panel is in LDS, the three passes run
            assert old["plan"] == new["plan"] and old["panel_flag"] == new["panel_flag"], label
            zc.same_bits(new, old, ESTEP_OUT)
            # what the variant is there for, read from the dense form
            p_vl, p_v, s = old["p_vl"], old["p_v"], old["s"]
            assert s.min() >= 1e-200
            if variant in ("mixed", "small_s"):
                fin = p_vl[:, np.isfinite(p_vl).all(0)]                # (the line without a direction is NaN under "angle")
                if (fin == 0).any() and (fin > 0).any():
                    seen.add("zeros")
                if (fin.sum(0) == 0).any():
                    seen.add("floored line")
            if variant == "big_s" and measure == "dotprod":
                assert (p_vl > 0).all(), label                         # nothing underflows: every VP is kept
            if variant == "inf_vp" and measure == "angle":
                assert np.isnan(old["lvsq"][0]).all() and np.isnan(p_vl).all(), label
            if variant == "nan_map":
                assert (p_v == 0).all() and not (p_vl > 0).any(), label     # no component is listed: every term is 0
            if variant == "nan_pv":
                k = min(1, m - 1)
                assert np.isnan(p_v[k]) and np.isfinite(np.delete(p_v, k)).all(), label
                assert np.isfinite(np.delete(old["lvsq"][k], 2)).all(), label      # (line 2 has no direction: NaN under "angle")
                assert np.isnan(p_vl).all(), label
            if variant == "mixed" and m >= len(zc.S_MIXED):
                assert (1e-200 in s) and (1e-6 in s) and (1e-3 in s), label
    assert {"zeros", "floored line"} <= seen, seen


def _em_both(sc, kw, measure):
    kw = dict(kw)
    init = kw.pop("init_vp", None)
    return [sim.em_single(sc["l"], sc["lp"], sc["cnn_response"], sc["sphere_image"], distance_measure=measure, smoother=mode,
                          init_vp=init, lds_doubles=BUDGET, **kw) for mode in (0, 1)]


@pytest.mark.parametrize("name", golden_cases())
def test_goldens_whole_em_angle(name):
    g = load(name)
    new, old = _em_both(g, em_kwargs(g), "angle")
    assert old["status"] == int(g["o_status"])
    assert (new["status"], new["iterations"], new["flags"]) == (old["status"], old["iterations"], old["flags"])
    zc.same_bits(new, old, EM_OUT)


@pytest.mark.parametrize("stem", dp.stems())
def test_goldens_whole_em_dotprod(stem):
    g, kw, r = dp.case(stem)
    new, old = _em_both(g, kw, "dotprod")
    assert old["iterations"] == int(r["o_iterations"])
    assert (new["status"], new["iterations"], new["flags"]) == (old["status"], old["iterations"], old["flags"])
    zc.same_bits(new, old, EM_OUT)
