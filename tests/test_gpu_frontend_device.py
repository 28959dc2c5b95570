"""The image front end on the GPU (vpk_image_prepare_batch + vpk_lsd_detect_batch + vpk_lsd_rows_to_lines,
frontend.lines_batch_device): the device resize and grey levels against the host build of the same source
(tests/hostsim/sim_frontend.cpp) and Pillow byte for byte; the lines against the host chain fed the device's grey levels
(lsd.detect_line_segments_batch -> detect_lsd_lines -> homogeneous_lines, the same detector kernels) byte for byte; the
batch contract (composition, chunking, workspace limit, overflow retry, mixed channels, argument rules); and the path on
to the sphere raster, the CNN and the EM, the pickles and example.py."""
import ctypes
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from test_frontend import _render
from test_gpu_lsd import _unmatched
from test_hostsim_frontend import _image, build_sim
from vanishing_points_2017_amd import _lib, frontend, lsd

pytestmark = pytest.mark.gpu

VPK_ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(seed, h, w, n=40, noise=2.0):
    """An RGB scene: strokes rendered per channel (a shared set and a set of the channel's own), with noise."""
    rs = np.random.RandomState(seed)
    shared = [tuple(rs.uniform(0, [w, h, w, h])) for _ in range(n)]
    chans = []
    for c in range(3):
        own = [tuple(rs.uniform(0, [w, h, w, h])) for _ in range(n // 4)]
        chans.append(_render(shared + own, h, w) * (0.7 + 0.15 * c) + rs.normal(0, noise, (h, w)))
    return np.clip(np.stack(chans, 2), 0, 255).astype(np.uint8)


@functools.lru_cache(None)
def _yud():
    return [_scene(s, 480, 640) for s in (1, 2, 3)]                # 640 x 480, no resize


@functools.lru_cache(None)
def _hlw():
    return [_scene(s, 1200, 1600, n=30) for s in (4, 5)]           # 1600 x 1200, target 800


@pytest.fixture(scope="module")
def sim():
    return build_sim()


@pytest.fixture(scope="module")
def rt():
    from vanishing_points_2017_amd.runtime import get_runtime
    return get_runtime(0)


def _prepare(rt, imgs, sizes, dims=None, in_off=None, out_off=None, resized=True):
    """Raw vpk_image_prepare_batch -> (rc, [resized], [grey])."""
    import torch
    n = len(imgs)
    d = np.array([[im.shape[1], im.shape[0], 1 if im.ndim == 2 else 3, s[0], s[1]] for im, s in zip(imgs, sizes)]
                 if dims is None else dims, dtype=np.int32).reshape(-1, 5)
    if in_off is None:
        in_off = np.r_[0, np.cumsum([im.size for im in imgs])]
    if out_off is None:
        out_off = np.r_[0, np.cumsum([s[0] * s[1] for s in sizes])]
    in_off, out_off = np.asarray(in_off, dtype=np.int64), np.asarray(out_off, dtype=np.int64)
    nbytes = sum(s[0] * s[1] * (1 if im.ndim == 2 else 3) for im, s in zip(imgs, sizes))
    flat = torch.from_numpy(np.concatenate([im.ravel() for im in imgs])).cuda()
    grey = torch.full((max(int(out_off[-1]), 1),), -1.0, dtype=torch.float64, device="cuda")
    res = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with rt.on_stream():
        rc = rt.lib.vpk_image_prepare_batch(rt.h, n, d.ctypes.data_as(ctypes.c_void_p), in_off.ctypes.data_as(ctypes.c_void_p),
                                            rt.ptr(flat), out_off.ctypes.data_as(ctypes.c_void_p),
                                            rt.ptr(res) if resized else None, rt.ptr(grey))
    rt.synchronize()
    if rc:
        return rc, None, None
    g, r = grey.cpu().numpy(), res.cpu().numpy()
    greys, outs, o = [], [], 0
    for k, (im, (w, h)) in enumerate(zip(imgs, sizes)):
        greys.append(g[out_off[k]:out_off[k + 1]].reshape(h, w))
        ch = 1 if im.ndim == 2 else 3
        outs.append(r[o:o + w * h * ch].reshape((h, w) if ch == 1 else (h, w, 3)))
        o += w * h * ch
    return 0, outs, greys


def _sizes(imgs, target):
    return [(im.shape[1], im.shape[0]) if target is None else frontend.fit_size(im.shape[1], im.shape[0], target)
            for im in imgs]


def _host_chain(greys):
    """The detector on the given grey levels, then detect_lsd_lines + homogeneous_lines on the host."""
    raw = lsd.detect_line_segments_batch(greys)
    segs, lines, nfa = [], [], []
    for g, r in zip(greys, raw):
        d = frontend.detect_lsd_lines(g, detector=lambda image, r=r: r)
        segs.append(d["segments"])
        lines.append(frontend.homogeneous_lines(d["segments"]))
        nfa.append(d["nfa"])
    offsets = np.r_[0, np.cumsum([len(s) for s in segs])].astype(np.int64)
    return offsets, np.concatenate(lines).reshape(-1, 3), np.concatenate(segs).reshape(-1, 4), np.concatenate(nfa)


def _host(res):
    return {k: (res[k].cpu().numpy() if k in ("l", "lp", "nfa", "sphere") else res[k]) for k in res if res[k] is not None}


def _same(a, b, keys=("l", "lp", "nfa")):
    assert np.array_equal(a["offsets"], b["offsets"])
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_device_resize_and_grey_equal_the_host_build_and_pillow(rt, sim):
    prepare, _ = sim
    rs = np.random.RandomState(1)
    cases = [(1600, 1200, 3, 800, 600), (2000, 1333, 3, 800, 533), (53, 37, 3, 640, 480), (7, 100, 1, 45, 640),
             (1000, 9, 3, 800, 7), (640, 480, 3, 640, 480), (640, 480, 1, 1, 1), (333, 250, 1, 333, 100),
             (1333, 2000, 3) + frontend.fit_size(1333, 2000, 800)]
    imgs = [_image(rs, w, h, ch) for w, h, ch, _, _ in cases]
    sizes = [(ow, oh) for _, _, _, ow, oh in cases]
    rc, outs, greys = _prepare(rt, imgs, sizes)
    assert rc == 0
    for img, (ow, oh), out, grey in zip(imgs, sizes, outs, greys):
        want, want_grey = prepare(img, ow, oh)
        assert np.array_equal(out, want) and grey.tobytes() == want_grey.tobytes()
        assert np.array_equal(out, np.asarray(Image.fromarray(img).resize((ow, oh), Image.LANCZOS)))
    # without the resized output: the same grey levels
    rc, _, greys2 = _prepare(rt, imgs, sizes, resized=False)
    assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(greys, greys2))


@pytest.fixture(scope="module", params=["yud_640x480", "hlw_1600x1200_to_800"])
def pinned(request, rt):
    imgs, target = (_yud(), None) if request.param.startswith("yud") else (_hlw(), 800)
    res = _host(frontend.lines_batch_device(imgs, target, keep_resized=True))
    rc, outs, greys = _prepare(rt, imgs, _sizes(imgs, target))
    assert rc == 0
    return imgs, target, res, outs, greys


def test_lines_equal_the_host_chain_on_the_device_grey(pinned):
    """The core pin: the same offsets, l, lp and -log10(NFA) bytes as the host chain fed the device's grey levels."""
    imgs, target, res, outs, greys = pinned
    offsets, l, lp, nfa = _host_chain(greys)
    assert offsets[-1] > 100 * len(imgs)
    _same(res, {"offsets": offsets, "l": l, "lp": lp, "nfa": nfa})
    assert res["image_shape"] == [g.shape for g in greys]
    assert all(np.array_equal(a, b) for a, b in zip(res["images"], outs))
    if target is not None:
        assert all(np.array_equal(a, frontend.resize_to_fit(im, target)) for a, im in zip(res["images"], imgs))


def _agreement(files, target):
    """(unmatched, total) segments of line_detector_batch against line_detector_device under test_gpu_lsd's rule."""
    want = frontend.line_detector_batch(files, target)
    got = frontend.line_detector_device(files, target)
    pad = lambda a: np.c_[a, np.zeros((len(a), 1)), np.ones((len(a), 2))]      # segments only: p = 0, nfa = 1
    total = bad = 0
    for (ia, sa), (ib, sb) in zip(want, got):
        assert np.array_equal(ia, ib)
        assert abs(len(sa) - len(sb)) <= max(2, len(sa) // 100)
        bad += _unmatched(pad(sb), pad(sa), tol=1e-6)
        total += len(sa)
    return bad, total


def test_agrees_with_line_detector_batch(tmp_path):
    """line_detector_batch's grey levels come from a BLAS dot, a few ulp away from the device's.  An ulp can flip one of the
    detector's discrete choices, and a changed region can change the later regions of the image, so
    rows are matched by test_gpu_lsd's rule (same place in the order +-2, coordinates within 1e-6) with a bound on the
    rows without a partner."""
    bad, total = _agreement(_pngs(tmp_path, _yud()[:2] + _hlw()[:1]), 800)
    # measured on the MI355X under this rule: 236 of 2366 segments (9.97 %) without a partner; the bound leaves room for
    # another BLAS build rounding the host's dot differently
    assert total > 300 and bad <= 12 * total // 100, (bad, total)


def test_independent_of_batch_composition_chunking_and_workspace(rt):
    imgs = [_yud()[0], _hlw()[0], _yud()[1][:, :, 0].copy(), _yud()[2]]
    full = _host(frontend.lines_batch_device(imgs, 800))
    # one image at a time, in another order
    singles = {k: _host(frontend.lines_batch_device([imgs[k]], 800)) for k in (3, 1, 0, 2)}
    for k in range(len(imgs)):
        lo, hi = full["offsets"][k], full["offsets"][k + 1]
        s = singles[k]
        assert hi - lo == s["offsets"][1]
        for key in ("l", "lp", "nfa"):
            assert full[key][lo:hi].tobytes() == s[key].tobytes()
    # chunked under max_pixels (one image per chunk), and with a small detector workspace
    _same(_host(frontend.lines_batch_device(imgs, 800, max_pixels=1)), full)
    _same(_host(frontend.lines_batch_device(imgs, 800, max_pixels=800 * 600 * 2)), full)
    rt.check(rt.lib.vpk_lsd_set_workspace_limit(rt.h, 4 << 20))
    try:
        _same(_host(frontend.lines_batch_device(imgs, 800)), full)
    finally:
        rt.check(rt.lib.vpk_lsd_set_workspace_limit(rt.h, 0))


def test_overflow_retry(monkeypatch):
    imgs = _yud()[:2] + [np.full((100, 120, 3), 90, np.uint8)]
    full = _host(frontend.lines_batch_device(imgs))
    assert np.diff(full["offsets"])[:2].min() > 10
    monkeypatch.setattr(frontend, "_DEVICE_CAP", 5)
    _same(_host(frontend.lines_batch_device(imgs, cnn_input_size=250)), full)


def test_mixed_channels_and_a_flat_image(rt):
    grey_img = _yud()[0][:, :, 1].copy()
    imgs = [_yud()[1], grey_img, np.full((300, 400, 3), 128, np.uint8), np.full((200, 200), 7, np.uint8), _hlw()[1]]
    res = _host(frontend.lines_batch_device(imgs, 640, keep_resized=True))
    counts = np.diff(res["offsets"])
    assert counts[2] == 0 and counts[3] == 0 and counts[0] > 100 and counts[1] > 100
    assert res["images"][1].ndim == 2 and res["images"][0].shape == (480, 640, 3)
    rc, _, greys = _prepare(rt, imgs, _sizes(imgs, 640))
    assert rc == 0
    offsets, l, lp, nfa = _host_chain(greys)
    _same(res, {"offsets": offsets, "l": l, "lp": lp, "nfa": nfa})


def test_argument_errors(rt):
    import torch
    img = np.zeros((10, 12, 3), np.uint8)
    assert _prepare(rt, [img], [(12, 10)], dims=[[12, 10, 2, 12, 10]])[0] == VPK_ERR_ARG      # channels
    assert _prepare(rt, [img], [(12, 10)], dims=[[12, 10, 4, 12, 10]])[0] == VPK_ERR_ARG
    assert _prepare(rt, [img], [(12, 10)], dims=[[12, 10, 3, 0, 10]])[0] == VPK_ERR_ARG       # side < 1
    assert _prepare(rt, [img], [(12, 10)], in_off=[0, 12 * 10])[0] == VPK_ERR_ARG              # bytes, not pixels
    assert _prepare(rt, [img], [(12, 10)], out_off=[0, 12 * 10 * 3])[0] == VPK_ERR_ARG
    assert _prepare(rt, [img], [(6, 5)], out_off=[0, 12 * 10])[0] == VPK_ERR_ARG
    assert rt.lib.vpk_image_prepare_batch(rt.h, 0, None, None, None, None, None, None) == 0
    # rows -> lines: a count above max_segments
    rows = torch.zeros((2, 4, 7), dtype=torch.float64, device="cuda")
    out = torch.zeros((20, 4), dtype=torch.float64, device="cuda")
    dims = np.array([[640, 480], [640, 480]], dtype=np.int32)
    for offs, want in (([0, 4, 9], VPK_ERR_ARG), ([0, 4, 8], 0), ([0, 0, 0], 0)):
        o = np.array(offs, dtype=np.int64)
        with rt.on_stream():
            assert rt.lib.vpk_lsd_rows_to_lines(rt.h, 2, dims.ctypes.data_as(ctypes.c_void_p), rt.ptr(rows), 4,
                                                o.ctypes.data_as(ctypes.c_void_p), rt.ptr(out), None, None) == want
    rt.synchronize()
    # the detector's own rule: sides >= 8
    with pytest.raises(_lib.VpkError):
        frontend.lines_batch_device([np.zeros((7, 40, 3), np.uint8)])
    with pytest.raises(_lib.VpkError):
        frontend.lines_batch_device([np.zeros((100, 700), np.uint8)], target_size=5)
    with pytest.raises(ValueError):
        frontend.lines_batch_device([np.zeros((100, 70, 4), np.uint8)])


def test_sphere_cnn_and_em_end_to_end(rt, pinned):
    """Device sphere = get_sphere_image of the host-chain lines; CNN -> EM on the device front end's buffers = the same
    on em.upload_batch of the host-chain scenes."""
    from vanishing_points_2017_amd import cnn, em, evaluation
    imgs, target, _, _, greys = pinned
    res = frontend.lines_batch_device(imgs, target, cnn_input_size=500)
    offsets, l, lp, _ = _host_chain(greys)
    sphere = res["sphere"].cpu().numpy()
    scenes = []
    for k in range(len(imgs)):
        lk = l[offsets[k]:offsets[k + 1]]
        assert np.array_equal(sphere[k], evaluation.get_sphere_image(lk, size=500, alpha=0.1))
        scenes.append({"l": lk, "lp": lp[offsets[k]:offsets[k + 1]]})
    net = cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0), runtime=rt)
    resp = net.forward(sphere)
    for s, r in zip(scenes, resp):
        s["cnn_response"], s["sphere_image"] = r, None
    import torch
    with rt.on_stream():
        cnn_dev = torch.from_numpy(np.ascontiguousarray(resp.reshape(-1, 400))).to(rt.tdev)
        l_work = res["l"].clone()                                    # the EM normalises its own copy
    got = em.em_batch_device(rt, res["offsets"], l_work, res["lp"], cnn_dev, res["sphere"])
    # the same front end in one chunk per image (the outputs joined on the device), handed straight to the EM on the
    # runtime's stream without a host read in between
    chunked = frontend.lines_batch_device(imgs, target, cnn_input_size=500, max_pixels=1)
    assert np.array_equal(chunked["offsets"], res["offsets"])
    with rt.on_stream():
        l_work_c = chunked["l"].clone()
    got_c = em.em_batch_device(rt, chunked["offsets"], l_work_c, chunked["lp"], cnn_dev, chunked["sphere"])
    d = em.upload_batch(rt, scenes)
    want = em.em_batch_device(rt, d["offsets"], d["l"], d["lp"], d["cnn"], d["sphere"])
    rt.synchronize()
    assert np.array_equal(d["sphere"].cpu().numpy(), sphere)
    assert np.array_equal(chunked["sphere"].cpu().numpy(), sphere)
    for g in (got, got_c):
        for key in ("num_vp", "status", "iterations", "vp", "sigma", "counts", "vp_assoc"):
            a, b = g[key].cpu().numpy(), want[key].cpu().numpy()
            if key in ("vp", "sigma", "counts"):
                nv = g["num_vp"].cpu().numpy()
                a = np.concatenate([a[i, :nv[i]].ravel() for i in range(len(nv))])
                b = np.concatenate([b[i, :nv[i]].ravel() for i in range(len(nv))])
            assert a.tobytes() == b.tobytes(), key
        assert (g["status"].cpu().numpy() == 0).all()


def _pngs(tmp_path, imgs):
    files = []
    for k, im in enumerate(imgs):
        f = str(tmp_path / ("img%d.png" % k))
        Image.fromarray(im).save(f)
        files.append(f)
    return files


def test_create_data_pickles_frontend_device(tmp_path, rt):
    from vanishing_points_2017_amd import evaluation
    imgs = [_yud()[0], _hlw()[0], _yud()[1][:, :, 2].copy()]
    files = _pngs(tmp_path, imgs)
    res = {}
    for tag, kw in (("gpu", {"lsd_device": 0}), ("frontend", {"frontend_device": 0})):
        dest = tmp_path / tag
        dest.mkdir()
        ds = {"image_files": files, "name": "t", "pickle_files": [str(dest / (os.path.basename(f) + ".pkl")) for f in files]}
        evaluation.create_data_pickles(ds, update=True, cnn_input_size=250, target_size=640, **kw)
        res[tag] = []
        for p in ds["pickle_files"]:
            with open(p, "rb") as fh:
                res[tag].append(pickle.load(fh))
    resized = [frontend.resize_to_fit(im, 640) for im in imgs]
    rc, _, greys = _prepare(rt, resized, [(r.shape[1], r.shape[0]) for r in resized])
    assert rc == 0
    offsets, l, lp, _ = _host_chain(greys)
    for k, (a, b) in enumerate(zip(res["gpu"], res["frontend"])):
        assert set(a) == set(b) and set(a["lines"]) == set(b["lines"])
        la, lb = a["lines"], b["lines"]
        assert la["image_shape"] == lb["image_shape"] and la["image_file"] == lb["image_file"]
        assert np.array_equal(la["image"], lb["image"]) and lb["image"].dtype == np.uint8
        assert lb["line_segments"].tobytes() == lp[offsets[k]:offsets[k + 1]].tobytes()
        assert lb["lines"].tobytes() == l[offsets[k]:offsets[k + 1]].tobytes()
        assert b["sphere_image"].shape == (250, 250) and b["sphere_image"].dtype == np.uint8
        assert np.array_equal(b["sphere_image"], evaluation.get_sphere_image(lb["lines"], size=250, alpha=0.1))
    ds = {"image_files": files, "name": "t", "pickle_files": [str(tmp_path / "x.pkl")] * 3}
    for kw in ({"lsd_device": 0}, {"line_detector": frontend.line_detector}, {"cnn_input_size": None}):
        with pytest.raises(ValueError):
            evaluation.create_data_pickles(ds, update=True, frontend_device=0, **kw)


def test_example_gpu_frontend(tmp_path):
    src = tmp_path / "src"
    src.mkdir()
    _pngs(src, [_yud()[0], _yud()[2]])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "vanishing_points_2017_amd.example", "--source_folder", str(src),
                        "--destination_folder", str(tmp_path / "dst"), "--lsd", "gpu-frontend"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if "line segments" in ln]
    assert len(lines) == 2 and all("640 x 480" in ln for ln in lines), p.stdout
