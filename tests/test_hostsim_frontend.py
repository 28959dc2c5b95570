"""The GPU image front end's PRODUCT arithmetic (csrc/image_device.hpp: Lanczos weights, the two integer resize passes,
the grey levels, rows -> lines) compiled for the host by tests/hostsim/sim_frontend.cpp and run serially: byte for byte
Pillow's Image.resize(LANCZOS) (frontend.resize_to_fit), the grey formula of include/vpk.h (vpk_image_prepare_batch)
and detect_lsd_lines + homogeneous_lines.  The kernels' orchestration is what tests/test_gpu_frontend_device.py covers."""
import ctypes

import numpy as np
import pytest
from PIL import Image

from hostsim import hostbuild
from vanishing_points_2017_amd import frontend


def build_sim():
    """The host build of tests/hostsim/sim_frontend.cpp; returns (prepare, rows_to_lines)."""
    lib = hostbuild.load("frontend")
    lib.sim_prepare.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    lib.sim_rows_to_lines.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_void_p]

    def prepare(image, out_w, out_h):
        """uint8 H x W (x 3) -> (resized uint8 image, fp64 grey levels) of the host build."""
        a = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = a.shape[:2]
        ch = 1 if a.ndim == 2 else 3
        res = np.zeros((out_h, out_w) if ch == 1 else (out_h, out_w, 3), dtype=np.uint8)
        grey = np.zeros((out_h, out_w))
        assert lib.sim_prepare(a.ctypes.data_as(ctypes.c_void_p), w, h, ch, out_w, out_h,
                               res.ctypes.data_as(ctypes.c_void_p), grey.ctypes.data_as(ctypes.c_void_p)) == 0
        return res, grey

    def rows_to_lines(rows, w, h):
        r = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 7)
        lp, l = np.zeros((r.shape[0], 4)), np.zeros((r.shape[0], 3))
        assert lib.sim_rows_to_lines(r.ctypes.data_as(ctypes.c_void_p), r.shape[0], w, h, lp.ctypes.data_as(ctypes.c_void_p),
                                     l.ctypes.data_as(ctypes.c_void_p)) == 0
        return lp, l
    return prepare, rows_to_lines


@pytest.fixture(scope="module")
def sim():
    return build_sim()


def grey_formula(image):
    """include/vpk.h, vpk_image_prepare_batch: the grey levels elementwise, left to right."""
    f = np.asarray(image).astype(np.float64)
    if f.ndim == 2:
        return (f / 255.0) * 255
    v = (f[..., 0] / 255.0) * 0.2125 + (f[..., 1] / 255.0) * 0.7154
    v = v + (f[..., 2] / 255.0) * 0.0721
    return v * 255


def _image(rs, w, h, ch):
    """Random pixels with smooth structure, saturated bands (the clip of both passes) and flat patches."""
    shape = (h, w) if ch == 1 else (h, w, 3)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 120 * np.sin(xx / 7.0 + yy / 11.0)
    if ch == 3:
        base = np.stack([base, 255 - base, np.full((h, w), 40.0)], 2)
    a = np.clip(base + rs.normal(0, 30, shape), 0, 255).astype(np.uint8)
    a[::9] = 255
    a[:, ::13] = 0
    return a


def _resize_cases():
    cases = [(1600, 1200, 800, 600), (2000, 1333, 800, 533), (53, 37, 640, 480), (7, 100, 45, 640), (1000, 9, 800, 7),
             (640, 480, 640, 480), (640, 480, 1, 1), (3, 2, 1, 1)]
    for w, h in ((640, 480), (2000, 1333), (1333, 2000)):
        for t in (640, 800):
            cases.append((w, h) + frontend.fit_size(w, h, t))
    return cases


@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("case", _resize_cases(), ids=lambda c: "%dx%d_to_%dx%d" % c)
def test_resize_is_pillows_lanczos_byte_for_byte(sim, case, ch):
    prepare, _ = sim
    w, h, ow, oh = case
    img = _image(np.random.RandomState(w * 7 + h + ch), w, h, ch)
    want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.LANCZOS))
    got, grey = prepare(img, ow, oh)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(grey, grey_formula(want))


def test_fit_size_is_resize_to_fits_shape():
    rs = np.random.RandomState(3)
    sizes = [(640, 480), (480, 640), (2000, 1333), (1333, 2000), (800, 800), (1, 1), (3000, 2), (2, 3000), (641, 479)]
    sizes += [tuple(rs.randint(1, 2500, 2)) for _ in range(40)]
    for w, h in sizes:
        for t in (250, 640, 800, 1000):
            img = np.zeros((h, w), dtype=np.uint8)
            nw, nh = frontend.fit_size(w, h, t)
            assert frontend.resize_to_fit(img, t).shape == (nh, nw), (w, h, t)


def test_grey_levels(sim):
    prepare, _ = sim
    rs = np.random.RandomState(5)
    rgb = rs.randint(0, 256, (97, 131, 3)).astype(np.uint8)
    rgb[0, :8] = [[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1], [254, 254, 254], [128, 64, 32]]
    _, grey = prepare(rgb, 131, 97)
    assert np.array_equal(grey, grey_formula(rgb))
    # frontend.rgb2gray's np.dot rounds the same sum in a BLAS-dependent order: within a few ulp of it
    want = frontend._detector_input(frontend.rgb2gray(rgb))
    ulp = np.abs(grey - want) / np.spacing(np.maximum(np.abs(want), 1e-300))
    assert ulp.max() <= 4, ulp.max()
    g = rs.randint(0, 256, (50, 70)).astype(np.uint8)
    _, grey = prepare(g, 70, 50)
    assert np.array_equal(grey, frontend._detector_input(frontend.rgb2gray(g)))


def _numpy_lines(rows, w, h):
    grey = np.full((h, w), 200.0)                         # detect_lsd_lines only reads the shape (max > 1: no rescale)
    r = frontend.detect_lsd_lines(grey, detector=lambda image: rows)
    return r["segments"], frontend.homogeneous_lines(r["segments"]), r["nfa"]


@pytest.mark.parametrize("w,h", [(640, 480), (480, 640), (800, 533), (9, 8), (1000, 1000)])
def test_rows_to_lines_is_numpys_byte_for_byte(sim, w, h):
    _, rows_to_lines = sim
    rs = np.random.RandomState(w + h)
    rows = np.c_[rs.uniform(-1, w + 1, (500, 1)), rs.uniform(-1, h + 1, (500, 1)), rs.uniform(-1, w + 1, (500, 1)),
                 rs.uniform(-1, h + 1, (500, 1)), rs.uniform(1, 3, (500, 1)), np.full((500, 1), 0.125),
                 rs.uniform(0, 50, (500, 1))]
    rows[:5, :4] = [[w / 2.0, h / 2.0, 0, 0], [0, h, w, 0], [w / 2.0, 0, w / 2.0, h], [1, 1, 1, 1], [0.5, h / 2.0, w, h / 2.0]]
    seg, lines, _ = _numpy_lines(rows, w, h)
    lp, l = rows_to_lines(rows, w, h)
    assert lp.tobytes() == np.ascontiguousarray(seg).tobytes()       # -0.0 included
    assert l.tobytes() == np.ascontiguousarray(lines).tobytes()


def test_rows_to_lines_of_an_empty_image(sim):
    _, rows_to_lines = sim
    seg, lines, _ = _numpy_lines(np.zeros((0, 7)), 640, 480)
    lp, l = rows_to_lines(np.zeros((0, 7)), 640, 480)
    assert lp.shape == seg.shape == (0, 4) and l.shape == lines.shape == (0, 3)
