"""The line segment detector's one source (csrc/lsd_device.hpp: Gaussian samples with host-made weights, gradient, seed
bins, region growing, rectangles, refinement, NFA; csrc/lsd_host.hpp: its serial loop with a one-lane wave) compiled by g++
through tests/hostsim/sim_lsd.cpp -- bit for bit the rows of the product's clang build of the same source, vpk_lsd_detect
(csrc/vpk_lsd.cpp), and, under the portable math policy, the rows recorded in tests/golden/lsd/lsd_portable.npz from the tree in
which the host detector was still written out on its own.  The kernels' own orchestration (grid-wide passes, the LDS
counting sort, the wave-split loops) is what tests/test_gpu_lsd.py covers.  The same source with the portable math policy
(sim_lsd_portable, lsd_portable_math.hpp) is what tests/test_gpu_lsd_exact.py pins the GPU to byte for byte; here it must
stay a faithful LSD: the detector contract of test_frontend.py, and the host detector's rows within the rule the ocml path
is held to.  Also: the argument checks of lsd.detect_line_segments_batch that need no GPU."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from hostsim import hostbuild
from test_frontend import _render
from vanishing_points_2017_amd import _lib, lsd

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.SO_PATH), reason="libvpk.so not built")


def build_sim(export="sim_lsd"):
    """The host build of tests/hostsim/sim_lsd.cpp; returns run(image, scale) -> the rows of `export` (sim_lsd: libm,
    sim_lsd_portable: the portable math policy), all of them however many."""
    fn = getattr(hostbuild.load("lsd"), export)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_int)]

    def run(image, scale):
        img = np.ascontiguousarray(image, dtype=np.float64)
        h, w = img.shape
        cap = 8192
        while True:
            out = np.zeros((cap, 7))
            n = ctypes.c_int(0)
            assert fn(img.ctypes.data_as(ctypes.c_void_p), w, h, scale, out.ctypes.data_as(ctypes.c_void_p), cap,
                      ctypes.byref(n)) == 0
            if n.value <= cap:
                return out[:n.value].copy()
            cap = n.value
    return run


@pytest.fixture(scope="module")
def sim():
    return build_sim()


@pytest.fixture(scope="module")
def sim_portable():
    return build_sim("sim_lsd_portable")


def _strokes(seed, n, h, w, noise):
    rs = np.random.RandomState(seed)
    segs = [tuple(rs.uniform(0, [w, h, w, h])) for _ in range(n)]
    return _render(segs, h, w) + rs.normal(0, noise, (h, w))


def _cases():
    rs = np.random.RandomState(7)
    true = [(40, 50, 300, 70), (60, 200, 280, 120), (150, 20, 170, 230), (20, 230, 120, 140), (200, 30, 310, 220)]
    yield "strokes_noise", _render(true, 256, 336) + np.random.RandomState(4).normal(0, 1.5, (256, 336))
    yield "strokes150_640x480", _strokes(1, 150, 480, 640, 2.0)
    yield "noise_200", rs.uniform(0, 255, (200, 200))
    yield "constant", np.full((120, 90), 117.0)
    yield "min_8x8", rs.uniform(0, 255, (8, 8))
    yield "odd_9x13", _render([(1, 1, 8, 12)], 13, 9)
    yield "odd_641x479", _strokes(2, 40, 479, 641, 1.0)


CASES = list(_cases())


@pytest.mark.parametrize("scale", [0.8, 1.0, 0.5])
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_device_source_on_the_host_equals_the_host_detector(sim, name, scale):
    image = dict(CASES)[name]
    want = lsd.detect_line_segments(image, scale=scale)
    got = sim(image, scale)
    assert got.shape == want.shape
    assert got.tobytes() == want.tobytes(), "rows differ: %s" % np.argwhere(got != want)[:5]
    if name == "constant":
        assert want.shape[0] == 0
    if name.startswith("strokes"):
        assert want.shape[0] > 20


GOLDEN = os.path.join(HERE, "golden", "lsd", "lsd_portable.npz")
GOLDEN_IMAGES = ("noise_8x8", "stroke_9x13", "strokes6_48x40", "strokes12_96x80", "strokes20_160x120")
GOLDEN_SCALES = (0.8, 1.0, 0.5)


def golden_lsd():
    """tests/golden/lsd/lsd_portable.npz (oracle/make_lsd_golden.py): name -> (image as float64, {scale: recorded rows})."""
    with np.load(GOLDEN) as z:
        return {name: (z["image_" + name].astype(np.float64), {s: z["rows_%s_%g" % (name, s)] for s in GOLDEN_SCALES})
                for name in GOLDEN_IMAGES}


@pytest.mark.parametrize("scale", GOLDEN_SCALES)
@pytest.mark.parametrize("name", GOLDEN_IMAGES)
def test_portable_build_equals_the_recorded_rows(sim_portable, name, scale):
    image, rows = golden_lsd()[name]
    want = rows[scale]
    got = sim_portable(image, scale)
    assert got.shape == want.shape
    assert got.tobytes() == want.tobytes(), "rows differ: %s" % np.argwhere(got != want)[:5]
    assert want.shape[0] >= 5 if name.startswith("strokes") else want.shape[0] == (2 if name == "stroke_9x13" else 0)


def test_a_nan_pixel_is_binned_in_range(sim):
    """grad_bin clamps the bin of a NaN magnitude, on the host as in lsd_order's LDS histogram: the call returns VPK_OK
    (detect_line_segments raises otherwise) with finite rows, the g++ build's."""
    image = golden_lsd()["strokes6_48x40"][0]
    image[20, 24] = np.nan
    for scale in GOLDEN_SCALES:
        got = lsd.detect_line_segments(image, scale=scale)
        assert got.shape[0] >= 1 and np.isfinite(got).all()
        assert got.tobytes() == sim(image, scale).tobytes()


def test_batch_rejects_a_non_2d_image_before_device_work(monkeypatch):
    def no_handle(device=0):
        raise AssertionError("device work before the shape check")
    monkeypatch.setattr(_lib, "get_handle", no_handle)
    with pytest.raises(ValueError):
        lsd.detect_line_segments_batch([np.zeros((20, 20)), np.zeros((20, 20, 3))])


def test_batch_without_a_gpu_raises_vpk_error(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_lib, "_handles", {})
    with pytest.raises(_lib.VpkError):
        lsd.detect_line_segments_batch([np.zeros((20, 20))])


def test_portable_build_keeps_the_detector_contract(sim_portable):
    from test_frontend import _seg_dist
    rs = np.random.RandomState(4)
    true = [(40, 50, 300, 70), (60, 200, 280, 120), (150, 20, 170, 230), (20, 230, 120, 140), (200, 30, 310, 220)]
    det = sim_portable(_render(true, 256, 336) + rs.normal(0, 1.5, (256, 336)), 0.8)
    assert det.shape[1] == 7 and det.shape[0] >= 2 * len(true) - 2
    assert (det[:, 6] > 0).all() and np.allclose(det[:, 5], 0.125)
    for t in true:
        close = [d for d in det if _seg_dist(t, d)[0] <= 2.2 and _seg_dist(t, d)[1] <= 1.5]
        assert close, ("no detection along", t)
        assert sum(np.hypot(d[2] - d[0], d[3] - d[1]) for d in close) >= 1.2 * np.hypot(t[2] - t[0], t[3] - t[1])
    for d in det:
        assert min(_seg_dist(t, d)[0] for t in true) <= 3.0
    rs0 = np.random.RandomState(0)
    assert sum(sim_portable(rs0.uniform(0, 255, (200, 200)), 0.8).shape[0] for _ in range(3)) <= 1


def test_portable_build_agrees_with_the_host_detector(sim_portable):
    """The rule tests/test_gpu_lsd.py holds the device-libm path to, on the same 24 images: the portable functions differ
    from glibc's by about an ulp too, so they move the same rare rows across pixel boundaries."""
    from test_gpu_lsd import IMAGES, _unmatched
    with ThreadPoolExecutor(8) as pool:                        # ctypes calls release the GIL
        got = list(pool.map(lambda im: sim_portable(im, 0.8), IMAGES))
        want = list(pool.map(lambda im: lsd.detect_line_segments(im, scale=0.8), IMAGES))
    total = bad = same = 0
    for g, w in zip(got, want):
        assert abs(g.shape[0] - w.shape[0]) <= max(2, w.shape[0] // 200), (g.shape, w.shape)
        b = _unmatched(g, w)
        total += w.shape[0]
        bad += b
        same += g.shape == w.shape and b == 0
    assert total > 1000
    # measured: 98 of 30 008 rows without a partner, 12 of the 24 images equal in every row (the device libm: 674, 10)
    assert bad <= 3 * total // 100, (bad, total)
    assert same >= 8, same
