"""vpk_vp_order_batch, vpk_to_pixels_batch, calc_horizon.horizon_batch_device and detector.Detector on the GPU.

The two kernels are held exactly to the host build of their bodies (tests/test_detector.py: the stable order rule, NumPy's
pixel bytes) on that file's tables.  The horizon without a caller's order is held bit for bit to vpk_horizon_batch fed the
host's stable order, and to the reference's stored results wherever the order is unambiguous.  The detector is held bit for
bit, in every tensor, to the staged chain it composes: lines_batch_device, em_batch_device on the images with three or more
segments, the horizon with the stable order, the NumPy pixel formula."""
import functools

import numpy as np
import pytest

import test_detector as T
from test_frontend import _render
from test_gpu_horizon import ATOL, _random_results, end_point_error
from test_horizon_cases import FIELDS, load_cases, num_best, port

pytestmark = pytest.mark.gpu

VPK_ERR_ARG = -1
EM_KEYS = ("vp", "sigma", "counts", "counts_weighted", "num_vp", "vp_assoc", "iterations", "status", "flags")
ALL_KEYS = ("l", "lp", "nfa", "sphere", "cnn") + EM_KEYS + ("l_norm", "order", "horizon", "combo", "lp_px", "vp_px", "horizon_px")
MAXBEST = 20


@pytest.fixture(scope="module")
def rt():
    from vanishing_points_2017_amd.runtime import get_runtime
    return get_runtime(0)


@pytest.fixture(scope="module")
def sim():
    return T.build_sim()


def _dev(rt, a):
    return rt.torch.from_numpy(np.ascontiguousarray(a)).to(rt.tdev)


# ---- vpk_vp_order_batch -------------------------------------------------------------------------------------------------
def _order(rt, counts, num, maxbest):
    from vanishing_points_2017_amd import calc_horizon as ch
    with rt.on_stream():
        d_c, d_n = _dev(rt, counts), _dev(rt, num)
    out = ch.vp_order_batch_device(rt, d_c, d_n, maxbest)
    rt.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("maxbest", T.ORDER_MAXBEST)
def test_order_equals_the_stable_rule_on_the_cpu_table(rt, sim, maxbest):
    counts, num = T.order_table()
    got = _order(rt, counts, num, maxbest)
    assert got.dtype == np.int32 and got.shape == (len(num), maxbest)
    assert np.array_equal(got, T.order_want(counts, num, maxbest))
    assert np.array_equal(got, T.sim_order(sim, counts, num, maxbest))


def _ragged():
    """The ragged shape of test_gpu_horizon.py: 300 interleaved images of 0 to 64 VPs, counts with many ties."""
    sizes = [(0, 1, 2, 3, 20, 21, 64)[k % 7] for k in range(300)]
    results = _random_results(np.random.RandomState(5), sizes)
    vp, counts = np.zeros((300, 64, 3)), np.full((300, 64), 1e6)
    for b, r in enumerate(results):
        vp[b, :sizes[b]], counts[b, :sizes[b]] = r["vp"], r["counts"]
    return vp, counts, np.array(sizes, dtype=np.int32)


def test_order_of_300_interleaved_images(rt):
    _, counts, num = _ragged()
    assert any(len(np.unique(counts[b, :num[b]])) < num[b] for b in range(300))      # ties are present
    for maxbest in (64, 10):
        assert np.array_equal(_order(rt, counts, num, maxbest), T.order_want(counts, num, maxbest))


def test_order_argument_errors_leave_the_output_and_the_handle(rt):
    torch = rt.torch
    counts, num = T.order_table()
    batch = len(num)
    with rt.on_stream():
        d_c, d_n = _dev(rt, counts), _dev(rt, num)
        wide = _dev(rt, np.zeros((batch, 65)))

    def call(batch=batch, max_vp=64, maxbest=20, null=None, counts=d_c):
        with rt.on_stream():
            out = torch.full((max(batch, 1), max(maxbest, 1)), -7, dtype=torch.int32, device=rt.tdev)
            p = {"counts": rt.ptr(counts), "num": rt.ptr(d_n), "out": rt.ptr(out)}
            if null:
                p[null] = None
            rc = rt.lib.vpk_vp_order_batch(rt.h, batch, max_vp, p["counts"], p["num"], maxbest, p["out"])
        rt.synchronize()
        return rc, out.cpu().numpy()

    rc, good = call()
    assert rc == 0 and np.array_equal(good, T.order_want(counts, num, 20))
    for kw in (dict(max_vp=0), dict(max_vp=65, counts=wide), dict(maxbest=0), dict(maxbest=65), dict(batch=-1),
               dict(null="counts"), dict(null="num"), dict(null="out")):
        rc, out = call(**kw)
        assert rc == VPK_ERR_ARG, kw
        assert (out == -7).all(), kw
        rc, out = call()
        assert rc == 0 and np.array_equal(out, good), kw
    rc, out = call(batch=0)                                      # nothing to do
    assert rc == 0 and (out == -7).all()


# ---- horizon_batch_device -----------------------------------------------------------------------------------------------
def _horizon(rt, vp, counts, num, maxbest, theta_vmin=np.pi / 10, theta_z=np.pi / 4, order=None):
    from vanishing_points_2017_amd import calc_horizon as ch
    with rt.on_stream():
        d = [_dev(rt, a) for a in (vp, counts, num)]
        d_o = None if order is None else _dev(rt, order)
    r = ch.horizon_batch_device(rt, d[0], d[1], d[2], maxbest, theta_vmin, theta_z, order=d_o)
    rt.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def test_horizon_without_an_order_is_the_horizon_of_the_stable_order(rt):
    vp, counts, num = _ragged()
    for maxbest in (64, 10):
        want_order = T.order_want(counts, num, maxbest)
        got = _horizon(rt, vp, counts, num, maxbest)
        want = _horizon(rt, vp, counts, num, maxbest, order=want_order)
        assert np.array_equal(got["order"], want_order)
        assert got["out"].shape == (300, 15) and got["out"].tobytes() == want["out"].tobytes()
        assert np.array_equal(got["combo"], want["combo"])


def _unambiguous(c):
    """A condition on the inputs: no NaN count, and no two equal among the min(maxbest + 1, M) largest -- every sort
    then puts the same VPs in the same first maxbest places."""
    cn = c["counts"]
    if np.isnan(cn).any():
        return False
    k = min(c["maxbest"] + 1, cn.size)
    return np.unique(np.sort(cn)[::-1][:k]).size == k


def test_stored_reference_cases_with_an_unambiguous_order(rt):
    _, cases = load_cases()
    cases = [c for c in cases if _unambiguous(c)]
    assert len(cases) >= 74 and sum(c["vp"].shape[0] > 16 for c in cases) >= 11
    groups = {}
    for c in cases:
        groups.setdefault((c["maxbest"], c["theta_vmin"], c["theta_z"]), []).append(c)
    worst = 0.0
    for (mb, tv, tz), group in sorted(groups.items()):
        max_vp = max([1] + [c["vp"].shape[0] for c in group])
        vp, counts = np.zeros((len(group), max_vp, 3)), np.zeros((len(group), max_vp))
        num = np.array([c["vp"].shape[0] for c in group], dtype=np.int32)
        for b, c in enumerate(group):
            vp[b, :num[b]], counts[b, :num[b]] = c["vp"], c["counts"]
        got = _horizon(rt, vp, counts, num, mb, tv, tz)
        for b, c in enumerate(group):
            where = (c["k"], c["kind"])
            o, cb = got["out"][b], got["combo"][b]
            combo = cb if cb[2] >= 0 else cb[:2]
            if c["raised"] and num_best(c) >= 3:                 # as test_gpu_horizon.py: the first triplet, NaN end points
                assert np.array_equal(combo, np.argsort(c["counts"], kind="stable")[::-1][:3]), where
                assert np.isnan(o[0:3]).any() and np.isnan(o[3:6]).any(), where
                continue
            want = port(c) if c["raised"] else [c[f] for f in FIELDS] + [c["combo"]]
            assert np.array_equal(combo, np.asarray(want[5]).ravel()), where
            for f, lo, w in zip(FIELDS[2:], (6, 9, 12), want[2:5]):
                assert np.array_equal(o[lo:lo + 3], np.asarray(w, dtype=np.float64), equal_nan=True), where + (f,)
            err = max(end_point_error(o[0:3], want[0]), end_point_error(o[3:6], want[1]))
            assert err <= ATOL, where + (err,)
            worst = max(worst, err)
    print("largest end-point error against the reference over %d cases: %.3e" % (len(cases), worst))


# ---- vpk_to_pixels_batch ------------------------------------------------------------------------------------------------
def _pixels(rt, dims, offsets, lp, vp, num_vp, horizon, want=(True, True, True), null_inputs=False):
    torch = rt.torch
    batch, max_vp = vp.shape[0], vp.shape[1]
    with rt.on_stream():
        d_lp, d_vp, d_n, d_h = [_dev(rt, a) for a in (lp, vp, num_vp, horizon)]
        outs = [torch.full(s, -7.25, dtype=torch.float64, device=rt.tdev)
                for s in (tuple(lp.shape), (batch, max_vp, 2), (batch, 2, 2))]
        ins = [rt.ptr(d_lp), rt.ptr(d_vp), rt.ptr(d_n), rt.ptr(d_h)]
        if null_inputs:                                          # the inputs of an output that is not asked for
            ins = [ins[0] if want[0] else None, ins[1] if want[1] else None, ins[2] if want[1] else None,
                   ins[3] if want[2] else None]
        rc = rt.lib.vpk_to_pixels_batch(rt.h, batch, T._p(dims), T._p(offsets), ins[0], max_vp, ins[1], ins[2], ins[3],
                                        *[rt.ptr(o) if w else None for o, w in zip(outs, want)])
    rt.synchronize()
    return rc, [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("want", [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)])
def test_pixels_equal_the_host_build_byte_for_byte(rt, sim, want):
    table = T.pixel_table()
    host = T.sim_pixels(sim, *table)
    for null_inputs in (False, True):
        rc, got = _pixels(rt, *table, want=want, null_inputs=null_inputs)
        assert rc == 0
        for name, g, h, w in zip(("lp_px", "vp_px", "horizon_px"), got, host, want):
            if w:
                assert g.tobytes() == h.tobytes(), name
            else:
                assert (g == -7.25).all(), name                  # not written


def test_pixels_many_rows_and_argument_errors(rt, sim):
    """More rows than one sweep of the grid (4096 blocks of 256 threads), images without segments in between; then the
    argument errors, which launch nothing."""
    rs = np.random.RandomState(14)
    n = np.array([0, 700000, 0, 0, 450001, 3, 0], dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    dims = np.array([(640, 480), (427, 640), (1, 1), (5, 9), (1048576, 3), (64, 64), (3, 2)], dtype=np.int32)
    lp = rs.uniform(-1, 1, (int(offsets[-1]), 4))
    vp = rs.normal(size=(7, 64, 3))
    num_vp = np.array([64, 0, 1, 70, -2, 33, 5], dtype=np.int32)
    horizon = rs.uniform(-2, 2, (7, 15))
    assert lp.shape[0] > 4096 * 256
    rc, got = _pixels(rt, dims, offsets, lp, vp, num_vp, horizon)
    assert rc == 0
    for g, h in zip(got, T.sim_pixels(sim, dims, offsets, lp, vp, num_vp, horizon)):
        assert g.tobytes() == h.tobytes()
    small = T.pixel_table()
    rc, good = _pixels(rt, *small)
    assert rc == 0
    dims, offsets = small[0], small[1]
    zero_side, falling = dims.copy(), offsets.copy()
    zero_side[2, 1] = 0
    falling[2] = falling[1] - 1
    for bad in ((zero_side, offsets), (dims, falling)):
        rc, out = _pixels(rt, bad[0], bad[1], *small[2:])
        assert rc == VPK_ERR_ARG and all((o == -7.25).all() for o in out)
        rc, out = _pixels(rt, *small)
        assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(out, good))
    with rt.on_stream():
        keep = rt.torch.zeros(8, dtype=rt.torch.float64, device=rt.tdev)
    args = (T._p(dims), T._p(offsets), None, 8, None, None, None)
    assert rt.lib.vpk_to_pixels_batch(rt.h, len(dims), *args, rt.ptr(keep), None, None) == VPK_ERR_ARG     # lp_px without lp
    assert rt.lib.vpk_to_pixels_batch(rt.h, len(dims), *args, None, rt.ptr(keep), None) == VPK_ERR_ARG     # vp_px without vp
    assert rt.lib.vpk_to_pixels_batch(rt.h, len(dims), *args, None, None, rt.ptr(keep)) == VPK_ERR_ARG     # ... horizon
    assert rt.lib.vpk_to_pixels_batch(rt.h, -1, *args, None, None, None) == VPK_ERR_ARG
    assert rt.lib.vpk_to_pixels_batch(rt.h, 0, None, None, None, 8, None, None, None, None, None, None) == 0
    rt.synchronize()
    assert (keep.cpu().numpy() == 0).all()


# ---- the detector -------------------------------------------------------------------------------------------------------
SCENES = ((1, 120, 160, True), (2, 160, 120, False), (3, 200, 200, True))      # seed, height, width, RGB
STROKE = (10, 12, 54, 50)


def _scene_image(seed, h, w, rgb):
    from vanishing_points_2017_amd import synth
    sc = synth.make_scene(seed, 20, 3, aspect_h=float(h) / w if w >= h else 1.0)
    s, scale = sc["lp"], max(w, h)
    px = np.stack([s[:, 0] * scale / 2 + w / 2, -s[:, 1] * scale / 2 + h / 2,
                   s[:, 2] * scale / 2 + w / 2, -s[:, 3] * scale / 2 + h / 2], axis=1)
    g = _render(px, h, w)
    if rgb:
        g = np.stack([g, g * 0.9, g * 0.8], axis=-1)
    return np.clip(np.rint(g), 0, 255).astype(np.uint8), sc["cnn_response"].astype(np.float32)


@functools.lru_cache(maxsize=None)
def _batch():
    """([images], response maps B x 20 x 20): three rendered scenes, a flat image and a single stroke."""
    made = [_scene_image(*s) for s in SCENES]
    imgs = [m[0] for m in made] + [np.full((64, 64), 128, np.uint8),
                                   np.clip(np.rint(_render([STROKE], 64, 64)), 0, 255).astype(np.uint8)]
    rs = np.random.RandomState(15)
    resp = np.stack([m[1] for m in made] + [rs.uniform(0, 0.08, (20, 20)).astype(np.float32) for _ in range(2)])
    return imgs, resp


@pytest.fixture(scope="module")
def net(rt):
    from vanishing_points_2017_amd import cnn
    return cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0), runtime=rt)


def _host(d):
    out = {k: d[k].cpu().numpy() for k in ALL_KEYS}
    out["offsets"], out["image_shape"] = np.asarray(d["offsets"]), [tuple(s) for s in d["image_shape"]]
    return out


_detected = {}


def _detect(rt, net, target):
    """The batch through detect_device once per target size, shared by the tests below (nobody writes to it)."""
    if target not in _detected:
        from vanishing_points_2017_amd.detector import Detector
        imgs, resp = _batch()
        with rt.on_stream():
            d_resp = _dev(rt, resp)
        rt.synchronize()
        det = Detector(net, target_size=target, maxbest=MAXBEST)
        _detected[target] = (det, _host(det.detect_device(imgs, cnn_response=d_resp)))
    return _detected[target]


def _staged(rt, imgs, resp, target):
    """The chain the detector composes, stage by stage with the host in between: lines_batch_device; em_batch_device on the
    images with three or more segments (the others: the all-None result, num_vp 0, status 1, zeros); the stable order on
    the host, then vpk_horizon_batch; the NumPy pixel formula."""
    from vanishing_points_2017_amd import em, frontend
    fe = frontend.lines_batch_device(imgs, target, cnn_input_size=500)
    offs = np.asarray(fe["offsets"])
    batch, total = len(imgs), int(offs[-1])
    want = {k: fe[k].cpu().numpy() for k in ("l", "lp", "nfa", "sphere")}
    want["cnn"] = resp
    n = np.diff(offs)
    keep = [b for b in range(batch) if n[b] >= 3]
    want.update({"vp": np.zeros((batch, 64, 3)), "sigma": np.zeros((batch, 64)), "counts": np.zeros((batch, 64)),
                 "counts_weighted": np.zeros((batch, 64)), "num_vp": np.zeros(batch, np.int32),
                 "vp_assoc": np.full(max(total, 1), -1, np.int64), "iterations": np.zeros(batch, np.int32),
                 "status": np.ones(batch, np.int32), "flags": np.zeros(batch, np.int32), "l_norm": want["l"].copy()})
    if keep:
        rows = np.concatenate([np.arange(offs[b], offs[b + 1]) for b in keep])
        sub_off = np.concatenate(([0], np.cumsum(n[keep]))).astype(np.int64)
        with rt.on_stream():
            l_sub, lp_sub = _dev(rt, want["l"][rows]), _dev(rt, want["lp"][rows])
            d_cnn, d_sph = _dev(rt, resp[keep].reshape(-1, 400)), _dev(rt, want["sphere"][keep])
        out = em.em_batch_device(rt, sub_off, l_sub, lp_sub, d_cnn, d_sph)
        rt.synchronize()
        for k in EM_KEYS:
            if k != "vp_assoc":
                want[k][keep] = out[k].cpu().numpy()
        want["vp_assoc"][rows] = out["vp_assoc"].cpu().numpy()[:rows.size]
        want["l_norm"][rows] = l_sub.cpu().numpy()
    want["order"] = T.order_want(want["counts"], want["num_vp"], MAXBEST)
    hz = _horizon(rt, want["vp"], want["counts"], want["num_vp"], MAXBEST, order=want["order"])
    want["horizon"], want["combo"] = hz["out"], hz["combo"]
    dims = np.array([(w, h) for h, w in fe["image_shape"]], dtype=np.int32).reshape(batch, 2)
    want["lp_px"], want["vp_px"], want["horizon_px"] = T.numpy_pixels(dims, offs, want["lp"], want["vp"], want["num_vp"],
                                                                      want["horizon"])
    want["offsets"], want["image_shape"] = offs, [tuple(s) for s in fe["image_shape"]]
    return want


def _assert_same(got, want, where=()):
    assert np.array_equal(got["offsets"], want["offsets"]) and got["image_shape"] == want["image_shape"], where
    for k in ALL_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, where + (k,)
        assert got[k].tobytes() == want[k].tobytes(), where + (k,)


@pytest.mark.parametrize("target", [None, 128])
def test_detect_device_equals_the_staged_chain_in_every_tensor(rt, net, target):
    imgs, resp = _batch()
    _, got = _detect(rt, net, target)
    _assert_same(got, _staged(rt, imgs, resp, target), (target,))
    n = np.diff(got["offsets"])
    assert n[3] == 0 and 0 < n[4] < 3 and (n[:3] >= 3).all()     # flat; one stroke; the scenes
    good = [b for b in range(3) if got["status"][b] == 0 and got["num_vp"][b] >= 3]
    assert len(good) >= 2, (got["status"], got["num_vp"])
    for b in good:                                               # a real selection, not a fallback
        assert got["combo"][b, 2] >= 0 and np.isfinite(got["horizon_px"][b]).all()
        assert np.isfinite(got["vp_px"][b, :got["num_vp"][b]]).any()
    shapes = [(120, 160), (160, 120), (200, 200), (64, 64), (64, 64)] if target is None else \
             [(96, 128), (128, 96), (128, 128), (128, 128), (128, 128)]
    assert got["image_shape"] == shapes


@pytest.mark.parametrize("target", [None, 128])
def test_images_without_three_segments_get_the_all_none_result(rt, net, target):
    from vanishing_points_2017_amd import calc_horizon as ch
    _, got = _detect(rt, net, target)
    empty = ch.calculate_horizon_and_ortho_vp({"vp": np.zeros((0, 3)), "counts": np.zeros(0)}, maxbest=MAXBEST)
    assert np.array_equal(np.abs(empty[0]), [1, 0, 1]) and np.array_equal(np.abs(empty[1]), [1, 0, 1])
    for b in (3, 4):
        h, w = got["image_shape"][b]
        assert got["num_vp"][b] == 0 and got["status"][b] == 1 and got["iterations"][b] == 0
        lo, hi = got["offsets"][b], got["offsets"][b + 1]
        assert (got["vp_assoc"][lo:hi] == -1).all() and np.isnan(got["vp_px"][b]).all()
        for f, lo3, e in zip(FIELDS, (0, 3, 6, 9, 12), empty[:5]):
            assert np.array_equal(got["horizon"][b, lo3:lo3 + 3], np.asarray(e, dtype=np.float64)), (b, f)
        assert np.array_equal(got["combo"][b], [0, 0, -1])
        ends = sorted(got["horizon_px"][b].tolist())             # y = 0: the middle row, from edge to edge of the long side
        assert ends == [[w / 2.0 - max(w, h) / 2.0, h / 2.0], [w / 2.0 + max(w, h) / 2.0, h / 2.0]]


@pytest.mark.parametrize("target", [None, 128])
def test_each_image_alone_equals_its_rows_in_the_batch(rt, net, target):
    imgs, resp = _batch()
    det, got = _detect(rt, net, target)
    offs = got["offsets"]
    for b in range(len(imgs)):
        with rt.on_stream():
            d_resp = _dev(rt, resp[b:b + 1])
        rt.synchronize()
        one = _host(det.detect_device([imgs[b]], cnn_response=d_resp))
        lo, hi = int(offs[b]), int(offs[b + 1])
        assert np.array_equal(one["offsets"], [0, hi - lo]) and one["image_shape"] == [got["image_shape"][b]]
        for k in ALL_KEYS:
            if k in ("l", "lp", "nfa", "l_norm", "lp_px"):
                want = got[k][lo:hi]
            elif k == "vp_assoc":
                want = got[k][lo:hi] if hi > lo else np.full(1, -1, np.int64)
            else:
                want = got[k][b:b + 1]
            assert one[k].tobytes() == np.ascontiguousarray(want).tobytes(), (b, k)


def test_an_empty_list_works(rt, net):
    from vanishing_points_2017_amd.detector import Detector
    det = Detector(net, maxbest=MAXBEST)
    d = det.detect_device([])
    assert list(d["offsets"]) == [0] and d["image_shape"] == []
    for k, tail in (("l", (3,)), ("lp", (4,)), ("lp_px", (4,)), ("vp", (64, 3)), ("vp_px", (64, 2)), ("horizon", (15,)),
                    ("horizon_px", (2, 2)), ("combo", (3,)), ("order", (MAXBEST,)), ("cnn", (20, 20)), ("num_vp", ())):
        assert tuple(d[k].shape) == (0,) + tail, k
    assert det.detect([]) == []


def test_detect_returns_the_same_values_in_the_reference_schema(rt, net, monkeypatch):
    from vanishing_points_2017_amd import detector
    imgs, resp = _batch()
    det, got = _detect(rt, net, None)
    with rt.on_stream():
        d_resp = _dev(rt, resp)
    rt.synchronize()
    real = detector.Detector.detect_device
    monkeypatch.setattr(detector.Detector, "detect_device", lambda self, images: real(self, images, cnn_response=d_resp))
    res = det.detect(imgs)
    assert len(res) == len(imgs)
    offs = got["offsets"]
    for b, r in enumerate(res):
        lo, hi = int(offs[b]), int(offs[b + 1])
        m = int(got["num_vp"][b])
        assert sorted(r) == ["EM_result", "horizon", "horizon_px", "line_segments_px", "lines", "status", "vp_px"]
        assert r["status"] == got["status"][b]
        assert r["lines"]["image_shape"] == got["image_shape"][b]
        assert np.array_equal(r["lines"]["line_segments"], got["lp"][lo:hi]) and np.array_equal(r["lines"]["lines"], got["l"][lo:hi])
        assert np.array_equal(r["line_segments_px"], got["lp_px"][lo:hi])
        assert np.array_equal(r["horizon_px"], got["horizon_px"][b]) and np.array_equal(r["vp_px"], got["vp_px"][b, :m], equal_nan=True)
        assert len(r["horizon"]) == 6
        for lo3, v in zip((0, 3, 6, 9, 12), r["horizon"][:5]):
            assert np.array_equal(v, got["horizon"][b, lo3:lo3 + 3], equal_nan=True)
        c = got["combo"][b]
        assert np.array_equal(r["horizon"][5], c if c[2] >= 0 else c[:2]) and r["horizon"][5].dtype == np.int64
        e = r["EM_result"]
        if got["status"][b] != 0:
            assert e is None
            continue
        assert set(e) == {"status", "flags", "l", "vp_assoc", "vp", "counts", "counts_weighted", "count_id", "decision_metric",
                          "iterations", "distribution", "sigma"}                    # em.em_batch's keys
        assert e["count_id"] is None and e["decision_metric"] is None and e["distribution"] is None
        assert e["iterations"] == got["iterations"][b] and e["vp"].shape == (m, 3)
        for k, v in (("vp", got["vp"][b, :m]), ("counts", got["counts"][b, :m]), ("sigma", got["sigma"][b, :m]),
                     ("counts_weighted", got["counts_weighted"][b, :m]), ("vp_assoc", got["vp_assoc"][lo:hi]),
                     ("l", got["l_norm"][lo:hi])):
            assert np.array_equal(e[k], v), (b, k)
    assert res[3]["EM_result"] is None and res[4]["EM_result"] is None
    assert sum(r["EM_result"] is not None for r in res[:3]) >= 2


def test_without_a_response_the_net_runs_and_the_range_policy_holds(rt, net):
    from vanishing_points_2017_amd._lib import VpkRangeError
    from vanishing_points_2017_amd.detector import Detector
    imgs, _ = _batch()
    det = Detector(net, maxbest=MAXBEST, range_policy="raise")
    d = det.detect_device(imgs)
    want = net.forward_device(d["sphere"])
    rt.synchronize()
    net.check_range()
    assert tuple(d["cnn"].shape) == (len(imgs), 20, 20)
    assert d["cnn"].cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    n = np.diff(d["offsets"])
    status = d["status"].cpu().numpy()
    assert (status[n < 3] == 1).all() and d["horizon_px"].shape == (len(imgs), 2, 2)
    # conv2's input scaled far out of fp16's range: "raise" raises, "recompute_exact" answers with the exact maps
    good = net.activation_scales()
    hot = good.copy()
    hot[0] = good[0] * np.float32(2.0 ** 40)
    try:
        net.set_activation_scales(hot)
        with pytest.raises(VpkRangeError):
            det.detect_device(imgs)
        exact = Detector(net, maxbest=MAXBEST, range_policy="recompute_exact").detect_device(imgs)
        assert net.image_range_flags().all()
        assert np.isfinite(exact["cnn"].cpu().numpy()).all()
    finally:
        net.set_activation_scales(good)
        net.set_range_policy("raise")
        net.range_flags()


def test_example_detector_flag_prints_what_detect_returns(rt, net, tmp_path, capsys):
    """example.py --source_folder DIR --detector, in process: the lines run_folder prints, from Detector.detect with
    run_folder's settings, and nothing written next to the images."""
    from PIL import Image
    from vanishing_points_2017_amd import example, frontend
    from vanishing_points_2017_amd.detector import Detector
    imgs, _ = _batch()
    files = []
    for name, k in (("a_scene.png", 0), ("b_flat.png", 3)):
        files.append(str(tmp_path / name))
        Image.fromarray(imgs[k]).save(files[-1])
    got = example.main(["--source_folder", str(tmp_path), "--detector"])
    out = [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("no trained weights")]
    want = Detector(net, target_size=640, cnn_input_size=500, maxbest=20).detect([frontend.imread(f) for f in files])
    lines = []
    for f, r in zip(files, want):
        h, w = r["lines"]["image_shape"]
        lines.append("%s %d x %d, %d line segments" % (f, w, h, r["lines"]["line_segments"].shape[0]))
        if r["EM_result"] is None:
            lines.append("  no vanishing points")
        else:
            (x1, y1), (x2, y2) = r["horizon_px"]
            lines.append("  VPs: %d, iterations: %d, horizon: (%.1f, %.1f) - (%.1f, %.1f)" % (
                r["EM_result"]["vp"].shape[0], r["EM_result"]["iterations"], x1, y1, x2, y2))
    assert out == lines
    assert [r["lines"]["image_shape"] for r in want] == [(480, 640), (640, 640)] and want[1]["EM_result"] is None
    assert len(got) == 2 and [r["status"] for r in got] == [r["status"] for r in want]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a_scene.png", "b_flat.png"]
