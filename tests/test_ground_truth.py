"""ground_truth.py against the reference's own arithmetic (tests/golden/ground_truth/ground_truth.npz, made by
scripts/make_ground_truth_golden.py from the text of the reference's benchmark.py with Python 2's division): the fixture
files are written into tmp_path in the datasets' layouts -- scipy.io.savemat for the .mat files, plain text for the csv,
small Pillow images for the shapes -- and the loaders' output must equal the goldens bit for bit.  Also: the floor
divisions matter, a missing row gives None, a missing file gives no error, and benchmark.py's flag rules.  No GPU."""
import os

import numpy as np
import pytest

from vanishing_points_2017_amd import calc_horizon, ground_truth

HERE = os.path.dirname(os.path.abspath(__file__))
io = pytest.importorskip("scipy.io")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "ground_truth", "ground_truth.npz"))


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _image(path, width, height):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.new("RGB", (int(width), int(height))).save(path)


def write_yud(root, g):
    """YUD's layout: cameraParameters.mat and P<id>/P<id>.jpg with P<id>GroundTruthVP_CamParams.mat beside it."""
    os.makedirs(root, exist_ok=True)
    io.savemat(os.path.join(root, "cameraParameters.mat"),
               {"focal": g["yud_focal"], "pixelSize": g["yud_pixel_size"], "pp": g["yud_pp"]})
    files = []
    for k, vp in enumerate(g["yud_vp"]):
        image_id = "P%07d" % (1020171 + k)
        files.append(os.path.join(root, image_id, image_id + ".jpg"))
        _image(files[-1], 8, 8)
        io.savemat(os.path.join(root, image_id, image_id + "GroundTruthVP_CamParams.mat"), {"vp": vp})
    return files


def write_ecd(root, g):
    """ECD's layout: <name>.jpg, <name>VP.mat, <name>hor.mat; the images have the fixtures' odd sizes."""
    files = []
    for k, (w, h) in enumerate(g["ecd_size"]):
        base = os.path.join(root, "%03d" % k)
        files.append(base + ".jpg")
        _image(files[-1], w, h)
        io.savemat(base + "VP.mat", {"zenith": g["ecd_zenith"][k], "hor_points": g["ecd_hor_points"][k]})
        hz = g["ecd_horizon"][k]
        io.savemat(base + "hor.mat", {"horizon": hz.reshape(3, 1) if g["ecd_horizon_as_column"][k] else hz.reshape(1, 3)})
    return files


def write_hlw(root, g, with_images=True):
    """HLW's layout: metadata.csv, split/test.txt, images/<name>.  The fixture's fourth image has no metadata row."""
    os.makedirs(os.path.join(root, "split"), exist_ok=True)
    with open(os.path.join(root, "metadata.csv"), "w") as fp:
        fp.write("".join(",".join(row) + "\n" for row in g["hlw_rows"].tolist()))
    names = [os.path.basename(f) for f in g["hlw_files"].tolist()]
    with open(os.path.join(root, "split", "test.txt"), "w") as fp:
        fp.write("".join(n + "\n" for n in names))
    files = [os.path.join(root, "images", n) for n in names]
    if with_images:
        for f in files:
            _image(f, 8, 8)
    return files


def _errors(g, key, true_horizon):
    out = []
    for th, (w, h) in zip(true_horizon, g[key + "_image_size"]):
        out.append([calc_horizon.horizon_error(np.array([1.0, y1, 1.0]), np.array([-1.0, y2, 1.0]), th, (int(h), int(w)))
                    for y1, y2 in g["detected"]])
    return np.array(out)


def test_york_equals_the_reference_bit_for_bit(golden, tmp_path):
    files = write_yud(str(tmp_path / "YUD"), golden)
    K, S = ground_truth.york_camera(str(tmp_path / "YUD"))
    assert _same(K, golden["yud_K"]) and _same(S, golden["yud_S"])
    assert K[0, 2] == 13 and K[1, 2] == -11 and S[0, 0] == 2.0 / 640
    truth = [ground_truth.york_truth(f, K, S) for f in files]
    assert _same(np.stack([t[0] for t in truth]), golden["yud_true_vps"])
    assert _same(np.stack([t[1] for t in truth]), golden["yud_true_horizon"])
    assert _same(_errors(golden, "yud", [t[1] for t in truth]), golden["yud_errors"])


def _eurasian_true_division(g, k):
    """The ECD VPs as `from __future__ import division` would give them: NOT the reference's."""
    w, h = [int(x) for x in g["ecd_size"][k]]
    vps = np.ones((3, 3))
    vps[:, 0:2] = np.vstack([g["ecd_zenith"][k], g["ecd_hor_points"][k]])
    vps[:, 0] -= w / 2
    vps[:, 1] -= h / 2
    vps[:, 1] *= -1
    vps[:, 0:2] /= max(w, h) / 2
    return vps


def test_eurasian_equals_the_reference_bit_for_bit_and_floors(golden, tmp_path):
    files = write_ecd(str(tmp_path / "ECD"), golden)
    assert (golden["ecd_size"] % 2).any(axis=1).all() and (golden["ecd_size"] % 2).all(axis=1).any()    # odd sides; both odd
    assert golden["ecd_horizon_as_column"].any() and not golden["ecd_horizon_as_column"].all()
    assert (golden["ecd_floor_divisions"] == 3).all()
    truth = [ground_truth.eurasian_truth(f, w, h) for f, (w, h) in zip(files, golden["ecd_size"])]
    assert _same(np.stack([t[0] for t in truth]), golden["ecd_true_vps"])
    assert _same(np.stack([t[1] for t in truth]), golden["ecd_true_horizon"])
    assert _same(_errors(golden, "ecd", [t[1] for t in truth]), golden["ecd_errors"])
    differ = [not np.array_equal(_eurasian_true_division(golden, k), golden["ecd_true_vps"][k]) for k in range(len(files))]
    assert all(differ)                                           # every fixture image has an odd side: floor != true division


def test_horizon_equals_the_reference_bit_for_bit(golden, tmp_path):
    files = write_hlw(str(tmp_path / "HLW"), golden)
    rows = ground_truth.horizon_metadata(str(tmp_path / "HLW"))
    assert [r[0] for r in rows] == ["a1", "b2", "c3"]            # directory part and extension cut (:97-98)
    assert any("/" in r[0] and "." in r[0] for r in golden["hlw_rows"].tolist())
    truth = [ground_truth.horizon_truth(rows, f) for f in files]
    assert truth[3] is None and bool(golden["hlw_last_is_none"])
    assert _same(np.stack(truth[:3]), golden["hlw_true_horizon"])
    assert _same(_errors(golden, "hlw", truth[:3]), golden["hlw_errors"])


def test_load_ground_truth_fills_the_dataset(golden, tmp_path):
    for name, write, key in (("york", write_yud, "yud"), ("eurasian", write_ecd, "ecd")):
        root = str(tmp_path / name)
        files = write(root, golden)
        ds = ground_truth.load_ground_truth({"image_files": files + [os.path.join(root, "gone.jpg")]}, name, root)
        assert _same(np.stack(ds["true_horizon"][:-1]), golden[key + "_true_horizon"])
        assert _same(np.stack(ds["true_vps"][:-1]), golden[key + "_true_vps"])
        assert ds["true_horizon"][-1] is None and ds["true_vps"][-1] is None and ds["image_shape"][-1] is None
        want = [(8, 8)] * 2 if name == "york" else [(int(h), int(w)) for w, h in golden["ecd_size"]]
        assert ds["image_shape"][:-1] == want                    # (height, width) of the image FILE
    root = str(tmp_path / "HLW")
    files = write_hlw(root, golden)
    os.remove(files[1])                                          # a listed image that is not there: no error (:119-121)
    ds = ground_truth.load_ground_truth({"image_files": files}, "horizon", root)
    assert ds["true_horizon"][1] is None and ds["image_shape"][1] is None
    assert ds["true_horizon"][3] is None and ds["image_shape"][3] == (8, 8)      # no metadata row (:247)
    assert _same(ds["true_horizon"][0], golden["hlw_true_horizon"][0]) and _same(ds["true_horizon"][2], golden["hlw_true_horizon"][2])
    assert ds["true_vps"] == [None] * 4
    with pytest.raises(ValueError):
        ground_truth.load_ground_truth({"image_files": []}, "kitti", root)


def test_scorable_follows_the_reference_loop(golden, tmp_path):
    """The first `start` positions count whether or not they can be scored; files, pickles and rows that are missing drop
    out (benchmark.py:113-132, :247)."""
    from vanishing_points_2017_amd import benchmark
    root = str(tmp_path / "HLW")
    files = write_hlw(root, golden)
    pickles = [str(tmp_path / ("%d.pkl" % i)) for i in range(4)]
    for p in pickles[:3]:
        open(p, "wb").close()
    os.remove(files[0])
    ds = ground_truth.load_ground_truth({"image_files": files, "pickle_files": pickles}, "horizon", root)
    assert benchmark.scorable(ds, 0) == ([1, 2], 0)
    assert benchmark.scorable(ds, 2) == ([1, 2], 1)
    os.remove(pickles[2])
    assert benchmark.scorable(ds, 0) == ([1], 0) and benchmark.scorable(ds, 0, need_pickles=False) == ([1, 2], 0)
    sub = benchmark.subset(ds, [1, 2])
    assert sub["image_files"] == files[1:3] and len(sub["true_horizon"]) == 2 and len(ds["image_files"]) == 4


def test_a_missing_scipy_is_said_plainly(monkeypatch, tmp_path):
    import sys
    monkeypatch.setitem(sys.modules, "scipy", None)
    with pytest.raises(ImportError, match="scipy.io.loadmat"):
        ground_truth.york_camera(str(tmp_path))


def test_benchmark_flag_rules(capsys):
    from vanishing_points_2017_amd import benchmark
    args = benchmark.build_parser().parse_args(["--yud"])
    assert args.lsd == "host" and args.batch == 64 and not args.detector and args.save_overlays is None
    args = benchmark.build_parser().parse_args(["--ecd", "--detector", "--batch", "8", "--lsd", "gpu-frontend",
                                                "--save-overlays", "somewhere"])
    assert args.detector and args.batch == 8 and args.lsd == "gpu-frontend" and args.save_overlays == "somewhere"
    for bad, word in ((["--yud", "--detector", "--synthetic"], "--synthetic"), (["--hlw", "--detector", "--gpus", "2"], "--gpus")):
        with pytest.raises(SystemExit) as e:
            benchmark.main(bad)
        assert e.value.code == 2
        assert word in capsys.readouterr().err
    assert benchmark.target_size("york") is None and benchmark.target_size("eurasian") == 800 == benchmark.target_size("horizon")
    assert "NotImplementedError" not in open(benchmark.__file__).read()


def test_without_trained_weights_the_random_net_stands_in_and_a_line_says_so(monkeypatch, tmp_path, capsys):
    from vanishing_points_2017_amd import benchmark, cnn, config
    made = []

    class _Net(object):
        def __init__(self, weights, mean, device=0):
            made.append((weights, mean, device))

        def set_range_policy(self, policy):
            made.append(policy)

    monkeypatch.setattr(config, "cnn_weights_path", str(tmp_path / "none.caffemodel"))
    monkeypatch.setattr(cnn, "Net", _Net)
    monkeypatch.setattr(cnn, "synthetic_weights", lambda seed: "weights%d" % seed)
    monkeypatch.setattr(cnn, "synthetic_mean", lambda seed: "mean%d" % seed)
    assert isinstance(benchmark.make_net(3, "recompute_exact"), _Net)
    assert made == [("weights0", "mean0", 3), "recompute_exact"]
    assert "no trained weights" in capsys.readouterr().out
