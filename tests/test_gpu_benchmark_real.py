"""vpk_horizon_error_batch and vpk_auc against the host build of their bodies (tests/test_score_host.py, whose tables these
tests import), and benchmark.py's two real-dataset flows end to end on fabricated datasets in the three real layouts.

The errors kernel is held byte for byte; the AUC kernel gives np.sort's order and an AUC within 2 (n + 4) 2^-53 of the host
build (the bound test_score_host.py derives), with the same bits on every run.  The datasets are rendered stroke scenes
saved with Pillow: YUD as P*/P*.jpg with their .mat files, ECD with odd sides, HLW with split/test.txt and metadata.csv; 27
images leave two behind the 25 the reference skips.  The pickle flow's AUC equals calc_auc of the errors recomputed here
from the written pickles; the detector flow's errors equal horizon_error on Detector.detect's host results bit for bit.
The two flows are not compared with each other: they order equal VP counts differently."""
import os

import numpy as np
import pytest

import test_score_host as T
from test_gpu_detector import _scene_image

pytestmark = pytest.mark.gpu

VPK_ERR_ARG, VPK_ERR_LIMIT = -1, -5
GPU_AUC_N = (1, 63, 64, 65, 255, 256, 257, 1025, 2018)
START = {"york": 25, "eurasian": 25, "horizon": 0}
FLAG = {"york": "--yud", "eurasian": "--ecd", "horizon": "--hlw"}
COUNT = {"york": 27, "eurasian": 27, "horizon": 3}


@pytest.fixture(scope="module")
def rt():
    from vanishing_points_2017_amd.runtime import get_runtime
    return get_runtime(0)


@pytest.fixture(scope="module")
def sim():
    return T.build_sim()


@pytest.fixture(scope="module")
def net(rt):
    from vanishing_points_2017_amd import cnn
    return cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0), runtime=rt)


def _dev(rt, a):
    return rt.torch.from_numpy(np.ascontiguousarray(a)).to(rt.tdev)


# ---- vpk_horizon_error_batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (0, 1, 63, 64, 65, 1025))
def test_errors_equal_the_host_build_byte_for_byte(rt, sim, batch):
    from vanishing_points_2017_amd import calc_horizon as ch
    horizon, th, dims = T.error_table(batch)
    with rt.on_stream():
        d_h, d_t = _dev(rt, horizon), _dev(rt, th)
    got = ch.horizon_error_batch_device(rt, d_h, d_t, dims)
    rt.synchronize()
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (batch,)
    assert got.tobytes() == T.sim_errors(sim, horizon, th, dims).tobytes()
    assert got.tobytes() == T.numpy_errors(horizon, th, dims).tobytes()


def test_errors_argument_errors_launch_nothing(rt):
    horizon, th, dims = T.error_table(8)
    with rt.on_stream():
        d_h, d_t = _dev(rt, horizon), _dev(rt, th)
        keep = rt.torch.full((8,), -7.25, dtype=rt.torch.float64, device=rt.tdev)
    bad = dims.copy()
    bad[5, 0] = 0
    lib = rt.lib
    assert lib.vpk_horizon_error_batch(rt.h, 8, rt.ptr(d_h), rt.ptr(d_t), T._p(bad), rt.ptr(keep)) == VPK_ERR_ARG
    assert lib.vpk_horizon_error_batch(rt.h, -1, rt.ptr(d_h), rt.ptr(d_t), T._p(dims), rt.ptr(keep)) == VPK_ERR_ARG
    assert lib.vpk_horizon_error_batch(rt.h, 8, None, rt.ptr(d_t), T._p(dims), rt.ptr(keep)) == VPK_ERR_ARG
    assert lib.vpk_horizon_error_batch(rt.h, 0, None, None, None, None) == 0
    rt.synchronize()
    assert (keep.cpu().numpy() == -7.25).all()


# ---- vpk_auc ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", GPU_AUC_N)
def test_auc_equals_the_host_build_within_the_bound_and_repeats(rt, sim, n):
    from vanishing_points_2017_amd import auc
    for name, err, ref in T.auc_cases(n):
        rc, want_sorted, want = T.sim_auc(sim, err)
        assert rc == 0
        with rt.on_stream():
            d_err = _dev(rt, err)
        runs = [auc.calc_auc_device(rt, d_err, cutoff=T.CUTOFF) for _ in range(2)]
        got, got_sorted = runs[0][0], runs[0][1].cpu().numpy()
        assert got_sorted.tobytes() == want_sorted.tobytes(), name
        assert np.array_equal(got_sorted, np.sort(err), equal_nan=True), name
        assert np.float64(got).tobytes() == np.float64(runs[1][0]).tobytes(), name           # the same bits on every run
        assert runs[1][1].cpu().numpy().tobytes() == got_sorted.tobytes(), name
        if np.isnan(want):
            assert np.isnan(got), name
            continue
        assert abs(got - want) <= T.auc_bound(n), (name, got, want)
        assert abs(got - T.reference_auc(err, ref)) <= T.auc_bound(n), (name, got)


def test_auc_limits_are_refused(rt):
    from vanishing_points_2017_amd import _lib, auc
    torch = rt.torch
    with rt.on_stream():
        big = torch.zeros((65537,), dtype=torch.float64, device=rt.tdev)
        keep = torch.full((65537,), -7.25, dtype=torch.float64, device=rt.tdev)
        out = torch.full((1,), -7.25, dtype=torch.float64, device=rt.tdev)
    assert rt.lib.vpk_auc(rt.h, 0, rt.ptr(big), 0.25, rt.ptr(keep), rt.ptr(out)) == VPK_ERR_ARG
    assert rt.lib.vpk_auc(rt.h, 65537, rt.ptr(big), 0.25, rt.ptr(keep), rt.ptr(out)) == VPK_ERR_LIMIT
    assert rt.lib.vpk_auc(rt.h, 8, rt.ptr(big), 0.25, rt.ptr(big), rt.ptr(out)) == VPK_ERR_ARG      # in place
    rt.synchronize()
    assert (keep.cpu().numpy() == -7.25).all() and float(out.cpu()[0]) == -7.25
    with pytest.raises(_lib.VpkError):
        auc.calc_auc_device(rt, big[:0])
    with pytest.raises(_lib.VpkError):
        auc.calc_auc_device(rt, big)
    got, srt = auc.calc_auc_device(rt, big[:65536])                      # the largest n: every error 0, the curve's area 1 - 1/2n... summed
    assert abs(got - T.stable_calc_auc(np.zeros(65536))) <= T.auc_bound(65536) and (srt.cpu().numpy() == 0).all()


# ---- fabricated datasets ----------------------------------------------------------------------------------------------
def fabricate(name, root, count, seeds=4):
    """A dataset of ``count`` rendered stroke scenes in the real layout of ``name`` under ``root``, ground truth included
    (random, but well-formed: the flows are held to each other and to the loaders, not to an accuracy).  ``seeds`` distinct
    scenes are rendered and reused in turn, except that the last three images are scenes of their own."""
    from PIL import Image
    from scipy import io
    rs = np.random.RandomState(31)
    os.makedirs(root, exist_ok=True)
    rendered = {}

    def scene(k, h, w):
        seed = 100 + (k if k >= count - 3 else k % seeds)
        if (seed, h, w) not in rendered:
            rendered[(seed, h, w)] = _scene_image(seed, h, w, True)[0]
        return rendered[(seed, h, w)]

    if name == "york":
        io.savemat(os.path.join(root, "cameraParameters.mat"), {"focal": 6.0532, "pixelSize": 0.0090, "pp": np.array([307.55, 251.45])})
        for k in range(count):
            image_id = "P%07d" % (1010000 + k)
            os.makedirs(os.path.join(root, image_id))
            Image.fromarray(scene(k, 480, 640)).save(os.path.join(root, image_id, image_id + ".jpg"), quality=92)
            q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
            io.savemat(os.path.join(root, image_id, image_id + "GroundTruthVP_CamParams.mat"), {"vp": q})
    elif name == "eurasian":
        for k in range(count):
            w, h = ((321, 241), (319, 240), (320, 239), (241, 321))[k % 4]
            base = os.path.join(root, "%03d" % k)
            Image.fromarray(scene(k, h, w)).save(base + ".jpg", quality=92)
            hor_points = np.stack([[-rs.uniform(200, 900), h * rs.uniform(0.3, 0.6)], [w + rs.uniform(200, 900), h * rs.uniform(0.3, 0.6)]])
            horizon = np.cross(np.append(hor_points[0], 1.0), np.append(hor_points[1], 1.0))
            horizon /= np.linalg.norm(horizon[:2])
            io.savemat(base + "VP.mat", {"zenith": np.array([[w / 2.0, -rs.uniform(800, 3000)]]), "hor_points": hor_points})
            io.savemat(base + "hor.mat", {"horizon": horizon.reshape(3, 1) if k % 2 else horizon.reshape(1, 3)})
    else:
        os.makedirs(os.path.join(root, "split"))
        os.makedirs(os.path.join(root, "images"))
        names, rows = [], []
        for k in range(count):
            w, h = ((400, 300), (300, 400), (333, 333))[k % 3]
            names.append("hlw_%03d.jpg" % k)
            Image.fromarray(scene(k, h, w)).save(os.path.join(root, "images", names[-1]), quality=92)
            # the rows are in the ORIGINAL image's units (here twice the file's), end points at x = -+ width / 2
            rows.append("flickr/%s,%d,%d,%.3f,%.3f,%.3f,%.3f" % (names[-1], 2 * h, 2 * w, -w, rs.uniform(-0.3, 0.3) * h, w,
                                                                rs.uniform(-0.3, 0.3) * h))
        with open(os.path.join(root, "split", "test.txt"), "w") as fp:
            fp.write("\n".join(names) + "\n")
        with open(os.path.join(root, "metadata.csv"), "w") as fp:
            fp.write("\n".join(rows) + "\n")
    return root


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    base = tmp_path_factory.mktemp("datasets")
    return {name: fabricate(name, str(base / name), COUNT[name]) for name in ("york", "eurasian", "horizon")}


@pytest.fixture()
def configured(datasets, net, monkeypatch, tmp_path):
    """config's roots point at the fabricated sets, no trained weights are configured, and the module's random-init net
    stands in for the one make_net would build (ten seconds of weight generation per call otherwise)."""
    from vanishing_points_2017_amd import benchmark, config
    monkeypatch.setattr(config, "yud_path", datasets["york"])
    monkeypatch.setattr(config, "ecd_path", datasets["eurasian"])
    monkeypatch.setattr(config, "hlw_path", datasets["horizon"])
    monkeypatch.setattr(config, "cnn_weights_path", str(tmp_path / "none.caffemodel"))
    monkeypatch.setattr(config, "cnn_mean_path", str(tmp_path / "none.binaryproto"))
    monkeypatch.setattr(benchmark, "make_net", lambda device, cnn_range: net)
    return datasets


def _truth(name, root, result_dir):
    """The dataset dict of the run in result_dir (get_data_list reads it back) with the loaders' ground truth."""
    from vanishing_points_2017_amd import benchmark, evaluation, ground_truth
    ds = evaluation.get_data_list(root, os.path.join(result_dir, name), 'default_net', "", "0", dataset_name=name,
                                  **benchmark.EM_CONFIG)
    assert len(ds["image_files"]) == COUNT[name]
    return ground_truth.load_ground_truth(ds, name, root)


@pytest.mark.parametrize("name", ("york", "eurasian", "horizon"))
def test_pickle_flow_scores_what_its_pickles_say(rt, configured, tmp_path, name):
    from vanishing_points_2017_amd import auc, benchmark, calc_horizon as ch, evaluation
    rd = str(tmp_path / "results")
    overlays = str(tmp_path / "overlays")
    got = benchmark.main([FLAG[name], "--result_dir", rd, "--lsd", "gpu-frontend", "--update_datalist", "--update_datafiles",
                          "--run_cnn", "--run_em", "--save-overlays", overlays])
    ds = _truth(name, configured[name], rd)
    idx = list(range(START[name], COUNT[name]))
    data = [evaluation._load_pickle(ds["pickle_files"][i]) for i in idx]
    results = [d["EM_result"] if d["EM_result"]["vp"] is not None else {'vp': np.zeros((0, 3)), 'counts': np.zeros(0)} for d in data]
    hz = ch.calculate_horizon_batch(results, maxbest=20, theta_vmin=np.pi / 10)
    errs = np.array([ch.horizon_error(h[0], h[1], ds["true_horizon"][i], ds["image_shape"][i]) for h, i in zip(hz, idx)])
    assert np.isfinite(errs).all()
    assert got == auc.calc_auc(errs.copy(), cutoff=0.25)[0]
    assert sorted(os.listdir(overlays)) == sorted(
        os.path.splitext(os.path.basename(ds["image_files"][i]))[0] + s for i in idx for s in ("_overlay.png", "_sphere.png"))


@pytest.mark.parametrize("name", ("york", "eurasian", "horizon"))
def test_detector_flow_equals_detect_on_the_same_files(rt, net, configured, tmp_path, name):
    from vanishing_points_2017_amd import auc, benchmark, calc_horizon as ch, frontend
    from vanishing_points_2017_amd.detector import Detector
    rd = str(tmp_path / "results")
    runs = {}
    for batch in (2, 8, 64):
        args = benchmark.build_parser().parse_args([FLAG[name], "--result_dir", rd, "--detector", "--batch", str(batch)])
        res = benchmark.run_detector(args, name)
        runs[batch] = (res["auc"], res["errors"].cpu().numpy(), res["sorted_errors"].cpu().numpy(), res["image_files"])
    ds = _truth(name, configured[name], rd)
    idx = list(range(START[name], COUNT[name]))
    files = [ds["image_files"][i] for i in idx]
    assert runs[8][3] == files
    det = Detector(net, target_size=benchmark.target_size(name), cnn_input_size=500, maxbest=20, theta_vmin=np.pi / 10.,
                   **benchmark.EM_CONFIG)
    host = det.detect([frontend.imread(f) for f in files])
    want = np.array([ch.horizon_error(r["horizon"][0], r["horizon"][1], ds["true_horizon"][i], ds["image_shape"][i])
                     for r, i in zip(host, idx)])
    assert runs[8][1].tobytes() == want.tobytes()
    assert abs(runs[8][0] - auc.calc_auc(want.copy(), cutoff=0.25)[0]) <= T.auc_bound(len(idx))
    assert np.array_equal(runs[8][2], np.sort(want))
    for batch in (2, 64):                                       # chunks of 2 split HLW's three images
        assert np.float64(runs[batch][0]).tobytes() == np.float64(runs[8][0]).tobytes()
        assert runs[batch][1].tobytes() == runs[8][1].tobytes() and runs[batch][2].tobytes() == runs[8][2].tobytes()
    overlays = str(tmp_path / "overlays")
    assert benchmark.main([FLAG[name], "--result_dir", rd, "--detector", "--batch", "8", "--save-overlays", overlays]) == runs[8][0]
    assert sorted(os.listdir(overlays)) == sorted(os.path.splitext(os.path.basename(f))[0] + "_overlay.png" for f in files)
