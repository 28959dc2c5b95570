"""Whole BASELINE.json configs through the HIP path FROM THE LINES ALONE against the REFERENCE's own stored results.

tests/golden/full_c<config>.npz hold what the reference (sphere_mapping.sphere_line_plot -> vp_localisation.
expectation_maximisation -> calc_horizon, run in the build container by oracle/make_full_goldens.py exactly as
evaluation.py:175 and :332-350 chain them) made of EVERY line set of configs[1] (YUD-shape, 102 images = bench.py's
workload) and configs[2] (ECD-shape, 103), of the configs[0] image (N = 800) and of a 64-image subsample of configs[3]
(HLW-shape).  Here the scenes carry lines and a response map, nothing else: vpk_sphere_raster makes the raster, and
* every raster must hash to the reference's raster (integer work: bit-exact), and
* the EM on it must meet the bar per image: line->VP assignments bit-exact, same iteration count, same VP count and
  per-VP line counts, VP directions within 1e-4.

Images for which tests/golden/instability.npz holds a certificate are the ones where the REFERENCE's own answer is
not defined to the last bit of its inputs: oracle/make_instability_certificates.py re-ran the reference itself on each
image this test once failed on, with ONE input coordinate moved by ONE ulp, and recorded how far the reference's own
result moves (VPs beyond the 1e-4 bar, flipped assignments, other iteration counts).  Nothing is exempt by hand: an
image that misses the bar without a certificate fails the test, and for a certified image the test still asserts
everything its certificate shows to be stable and bounds the rest by what the reference does to itself.
"""
import numpy as np
import pytest

from golden_util import check_parity
from vanishing_points_2017_amd import parity, synth

pytestmark = pytest.mark.gpu


def _run(cfg):
    import os
    if not os.path.isfile(parity.golden_path(cfg)):
        pytest.skip("no stored reference results for config %d" % cfg)
    from vanishing_points_2017_amd import em as gem
    ref = parity.ReferenceResults(cfg)
    scenes = [next(synth.config_scenes(cfg, count=1, start=int(i))) for i in ref.index]
    for i, s in zip(ref.index, scenes):
        assert s["sphere_image"] is None                                  # lines only
        assert parity.input_sha(s) == ref.get(i)["input_sha"], \
            "config %d image %d: the generator produced other inputs than the reference saw" % (cfg, i)
    res = gem.em_batch(scenes)                                            # raster (vpk_sphere_raster) -> EM
    wrong = [int(i) for i, s in zip(ref.index, scenes) if parity.raster_sha(s["sphere_image"]) != ref.get(i)["raster_sha"]]
    assert not wrong, "config %d: the rasters of images %s differ from the reference's sphere_line_plot output" % (cfg, wrong[:10])
    return ref, scenes, res


def _check(cfg):
    ref, scenes, res = _run(cfg)
    cert = parity.instability_certificates()
    _, _, bad = check_parity(((cfg, int(i)), r, ref.get(i), cert.get((cfg, int(i)))) for i, r in zip(ref.index, res))
    bad = [(label[1], c) for label, c in bad]
    assert not bad, "config %d: %d of %d images miss the parity bar without an instability certificate: %s" % (
        cfg, len(bad), len(ref), bad[:5])
    return ref, res


def test_config2_yud_shape_all_102_images():
    ref, _ = _check(2)
    assert len(ref) == 102


def test_config3_ecd_shape_all_103_images():
    ref, _ = _check(3)
    assert len(ref) == 103


def test_config4_hlw_shape_subsample():
    ref, _ = _check(4)
    assert len(ref) >= 32


def test_config1_single_image_n800_through_the_reference_call_surface():
    """configs[0]: one image, N = 800, through vp_localisation.expectation_maximisation (example.py's path)."""
    import os
    if not os.path.isfile(parity.golden_path(1)):
        pytest.skip("no stored reference results for config 1")
    from vanishing_points_2017_amd import vp_localisation
    ref = parity.ReferenceResults(1)
    from vanishing_points_2017_amd import evaluation
    sc = next(synth.config_scenes(1, count=1))
    g = ref.get(0)
    assert sc["lp"].shape[0] == 800 and parity.input_sha(sc) == g["input_sha"]
    sphere = evaluation.get_sphere_image(sc["l"], size=500, alpha=0.1)       # evaluation.py:175
    assert parity.raster_sha(sphere) == g["raster_sha"]
    l = sc["l"].copy()
    res = vp_localisation.expectation_maximisation(l, sc["lp"].copy(), sc["cnn_response"], sphere_image=sphere)
    res = dict(res, status=0 if res["vp"] is not None else 1)
    c = parity.compare_one(res, g)
    assert parity.passes(c), c
    assert np.allclose(np.linalg.norm(l, axis=1), 1.0)          # l normalised in place (:185-186)


def test_horizon_auc_equals_the_reference_on_config2():
    """The 'horizon-AUC parity' half of the metric: errors of images 26..102 (benchmark.py:69) from the GPU
    EM + GPU horizon selection vs the reference's stored horizons, same synthetic ground truth."""
    from vanishing_points_2017_amd import auc as auc_mod, calc_horizon as ch
    ref, scenes, res = _run(2)
    cert = parity.instability_certificates()
    todo = [(int(i), s, r) for i, s, r in zip(ref.index, scenes, res) if int(i) >= 25 and r["status"] == 0]
    horizons = ch.calculate_horizon_batch([r for _, _, r in todo], maxbest=20, theta_vmin=np.pi / 10)
    e_gpu, e_ref = [], []
    for (i, s, _), h in zip(todo, horizons):
        g = ref.get(i)
        e_gpu.append(ch.horizon_error(h[0], h[1], s["true_horizon"], s["image_shape"]))
        e_ref.append(ch.horizon_error(g["hP1"], g["hP2"], s["true_horizon"], s["image_shape"]))
        if not cert.get((2, i), {}).get("unstable", False):             # (a certificate that says "stable" exempts nothing)
            assert np.array_equal(np.asarray(h[5]), g["combo"]), i       # same orthogonal triplet
            assert abs(e_gpu[-1] - e_ref[-1]) <= 1e-6, i
    a_gpu = auc_mod.calc_auc(np.array(e_gpu), cutoff=0.25)[0]
    a_ref = auc_mod.calc_auc(np.array(e_ref), cutoff=0.25)[0]
    assert abs(a_gpu - a_ref) <= 1e-4, (a_gpu, a_ref)


@pytest.mark.parametrize("seed", [5002, 5003, 5004])
def test_config5_stress_unit_against_the_oracle(seed):
    """configs[4]: the stress unit (1000 lines, 8 supplied VP candidates, 50 forced iterations, no split / merge) on
    fresh seeds against the CPU oracle (the reference needs ~40 s per such image; two of them are goldens:
    stress_n1000, stress_n300).  Same bar: assignments bit-exact, VPs within 1e-4."""
    from oracle import em_numpy
    from vanishing_points_2017_amd import em as gem
    from golden_util import gpu_rasters
    sc = gpu_rasters([synth.make_scene(seed, 1000, 8)])[0]
    sc["init_vp"] = synth.stress_init_vps(seed)
    kw = dict(num_iter=50, do_split=False, do_merge=False, final_convergence=-1)
    ref = em_numpy.expectation_maximisation(sc["l"].copy(), sc["lp"].copy(), sc["cnn_response"].copy(),
                                            sphere_image=sc["sphere_image"], init_vp=sc["init_vp"], **kw)
    res = gem.em_batch([sc], **kw)[0]
    assert res["status"] == 0 and res["iterations"] == ref["iterations"] == 49
    assert res["vp"].shape == ref["vp"].shape
    assert np.array_equal(res["vp_assoc"], ref["vp_assoc"])
    assert np.abs(res["vp"] - ref["vp"]).max() <= 1e-4
    assert np.array_equal(res["counts"], ref["counts"])
