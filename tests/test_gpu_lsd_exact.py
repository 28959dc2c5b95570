"""vpk_lsd_detect_batch pinned bit for bit: with the portable math policy (vpk_lsd_set_math(h, 1), lsd_portable_math.hpp)
the device and the host build of lsd_device.hpp (tests/hostsim/sim_lsd.cpp: sim_lsd_portable) call the same elementary
functions, so every row of every image must be equal byte for byte -- counts and tobytes(), no tolerance.  What this pins
is the device orchestration the tolerant test of tests/test_gpu_lsd.py cannot see: the grid-wide passes, the atomicMax of
the max gradient, the counting sort with ballot ranks across the waves of lsd_order, the 64-lane split of rect_nfa and
region2rect, the chunking and the overflow rule -- at the batch's scales (0.8, 1.0 without sub-sampling, 0.5, 1.25
up-sampling), at edge shapes, on long rectangles spanning far more than 64 columns and rows, and on exact gradient ties."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_frontend import _render
from test_gpu_lsd import IMAGES, _Dev, _strokes
from test_hostsim_lsd import GOLDEN_IMAGES, GOLDEN_SCALES, build_sim, golden_lsd

pytestmark = pytest.mark.gpu

VPK_ERR_ARG = -1


@pytest.fixture(scope="module")
def port():
    run = build_sim("sim_lsd_portable")

    def rows(images, scale):
        with ThreadPoolExecutor(8) as pool:                   # ctypes calls release the GIL
            return list(pool.map(lambda im: run(im, scale), images))
    return rows


@pytest.fixture(scope="module")
def dev():
    d = _Dev()
    yield d
    d.h.check(d.h.lib.vpk_lsd_set_math(d.h.h, 0))         # the handle is shared with the other GPU tests
    d.set_limit(0)


def _set_math(dev, mode):
    dev.h.check(dev.h.lib.vpk_lsd_set_math(dev.h.h, mode))


def _assert_rows(tag, got, n, want, cap=None):
    """Image `tag`'s device rows (got: its full output slot, n: its count) against the host build's, byte for byte; with
    a capacity, the first `cap` rows of the host's, and the slot untouched past what was written."""
    cap = got.shape[0] if cap is None else cap
    assert n == want.shape[0], "%s: %d rows on the device, %d on the host" % (tag, n, want.shape[0])
    k = min(n, cap)
    g, w = got[:k], want[:k]
    if g.tobytes() != w.tobytes():
        i = int(np.argwhere((g != w) | (np.isnan(g) != np.isnan(w)))[0][0])
        raise AssertionError("%s: first differing row %d of %d\n device %r\n host   %r" % (tag, i, k, g[i].tolist(),
                                                                                           w[i].tolist()))
    assert (got[k:] == -7.0).all(), "%s: written past the count (%d rows)" % (tag, k)


def _check(dev, port, images, scale, names=None, want=None, cap=None):
    want = port(images, scale) if want is None else want
    if cap is None:
        cap = max([w.shape[0] for w in want] + [1])
    _set_math(dev, 1)
    rc, out, n = dev.call(images, scale=scale, cap=cap)
    assert rc == 0
    names = names or ["image %d" % k for k in range(len(images))]
    for k, w in enumerate(want):
        _assert_rows("%s at scale %g" % (names[k], scale), out[k], int(n[k]), w, cap)
    return want


@pytest.fixture(scope="module")
def host_rows_08(port):
    return port(IMAGES, 0.8)


@pytest.mark.parametrize("scale", [0.8, 1.0, 0.5, 1.25])
def test_batch_equals_the_portable_host_build(dev, port, host_rows_08, scale):
    want = _check(dev, port, IMAGES, scale, want=host_rows_08 if scale == 0.8 else None)
    assert sum(w.shape[0] for w in want) > 1000


@pytest.mark.parametrize("scale", GOLDEN_SCALES)
def test_batch_equals_the_recorded_rows(dev, scale):
    """One call over the stored images of tests/golden/lsd/lsd_portable.npz: the rows recorded from the host, byte for byte."""
    gold = golden_lsd()
    _check(dev, None, [gold[name][0] for name in GOLDEN_IMAGES], scale, names=list(GOLDEN_IMAGES),
           want=[gold[name][1][scale] for name in GOLDEN_IMAGES])


def _edge_images():
    rs = np.random.RandomState(21)
    yy, xx = np.mgrid[0:300, 0:400]
    strokes = _strokes(22, 40, 300, 400, 1.0)
    strip_h = np.where(np.arange(3000)[None, :] % 400 < 200, 200.0, 30.0) + rs.normal(0, 2.0, (8, 3000))
    strip_v = np.where(np.arange(3000)[:, None] % 300 < 150, 180.0, 20.0) + rs.normal(0, 2.0, (3000, 8))
    return [("8x8", rs.uniform(0, 255, (8, 8))), ("strip_8x3000", strip_h), ("strip_3000x8", strip_v),
            ("constant", np.full((64, 96), 117.0)),
            ("below_rho", xx * 1.0 + yy * 1.5),                # |gradient| <= 1.3 < rho = 5.2 everywhere: no seed
            ("around_1e6", strokes * 4000.0 + 1e6), ("negative", -strokes - 500.0),
            ("step_noise", np.where(xx > 0.4 * yy + 150, 150.0, 90.0) + rs.normal(0, 4.0, (300, 400)))]


@pytest.mark.parametrize("scale", [0.8, 1.0])
def test_edge_shapes_and_values(dev, port, scale):
    names, images = zip(*_edge_images())
    want = _check(dev, port, list(images), scale, names=list(names))
    assert want[names.index("constant")].shape[0] == 0 and want[names.index("below_rho")].shape[0] == 0
    assert want[names.index("around_1e6")].shape[0] > 10 and want[names.index("negative")].shape[0] > 10


@pytest.mark.parametrize("scale", [0.125, 0.2, 0.3])
def test_a_scaled_side_of_one_two_or_three_pixels(dev, port, scale):
    names, images = zip(*_edge_images())
    _check(dev, port, list(images), scale, names=list(names))


def _long_images():
    h, w = 1500, 2000
    yy, xx = np.mgrid[0:h, 0:w]
    rs = np.random.RandomState(31)
    long_strokes = _render([(30, 40, 1960, 1400), (50, 1450, 1900, 100), (20, 700, 1980, 760), (1000, 10, 1040, 1490),
                            (100, 300, 1800, 320)], h, w, width=4.0) + rs.normal(0, 1.0, (h, w))
    step = np.where(yy > 600, 170.0, 60.0) + rs.normal(0, 2.0, (h, w))     # one edge across the whole width
    return [("long_strokes_2000x1500", long_strokes), ("step_edge_2000x1500", step)]


@pytest.mark.parametrize("scale", [0.8, 1.0])
def test_long_rectangles_beyond_a_wave(dev, port, scale):
    names, images = zip(*_long_images())
    strokes, step = _check(dev, port, list(images), scale, names=list(names))
    # rectangles spanning far more than 64 columns and 64 rows; the step's edge is one region across the width
    assert ((np.abs(strokes[:, 2] - strokes[:, 0]) > 256) & (np.abs(strokes[:, 3] - strokes[:, 1]) > 256)).any()
    assert (np.abs(step[:, 2] - step[:, 0]) > 400).any()


def _tie_images():
    yy, xx = np.mgrid[0:480, 0:640]
    rs = np.random.RandomState(41)
    return [("ramp", (xx * 3 + yy * 2) % 256 * 1.0),          # one gradient almost everywhere: one bin, every wave
            ("ramp_steep", xx * 9.0 + yy * 4.0),
            ("stripes", np.where(xx % 7 < 3, 200.0, 40.0)),
            ("stripes_diag", np.where((xx + yy) % 11 < 5, 220.0, 10.0)),
            ("checker", np.where((xx // 5 + yy // 5) % 2 == 0, 250.0, 0.0)),
            ("levels", rs.randint(0, 4, (480, 640)) * 60.0)]


@pytest.mark.parametrize("scale", [1.0, 0.8])
def test_exact_gradient_ties_across_the_order_waves(dev, port, scale):
    names, images = zip(*_tie_images())
    _check(dev, port, list(images), scale, names=list(names))


def test_chunking_batch_order_and_overflow(dev, port, host_rows_08):
    want = host_rows_08
    try:
        for limit in (1, 30 << 20):                            # one image per chunk / a few images per chunk
            dev.set_limit(limit)
            _check(dev, port, IMAGES, 0.8, names=["image %d, limit %d" % (k, limit) for k in range(len(IMAGES))],
                   want=want)
    finally:
        dev.set_limit(0)
    sub = [1, 13, 0, 22, 5, 10, 23, 9]                         # ragged, reordered
    _check(dev, port, [IMAGES[k] for k in sub], 0.8, names=["image %d (reordered)" % k for k in sub],
           want=[want[k] for k in sub])
    _check(dev, port, IMAGES, 0.8, names=["image %d, max_segments 7" % k for k in range(len(IMAGES))], want=want, cap=7)
    _set_math(dev, 1)
    rc, out, n = dev.call(IMAGES, scale=0.8, cap=0)
    assert rc == 0 and list(n) == [w.shape[0] for w in want]
    assert (out == -7.0).all()                                 # max_segments 0: nothing written


def test_mode_switch_and_arguments(dev, port):
    images = [IMAGES[k] for k in (0, 3, 12, 23)]
    _set_math(dev, 0)
    rc, ref, nref = dev.call(images)
    assert rc == 0
    _check(dev, port, images, 0.8)
    _set_math(dev, 1)
    rc, port_out, nport = dev.call(images)
    _set_math(dev, 0)
    rc, again, nagain = dev.call(images)
    assert rc == 0 and np.array_equal(nagain, nref)
    for k in range(len(images)):                               # mode 0 is the product's path, bit for bit
        assert again[k, :nref[k]].tobytes() == ref[k, :nref[k]].tobytes()
    # the hook changes the functions: the device libm differs from the portable ones somewhere in these rows
    assert any(nport[k] != nref[k] or port_out[k, :nref[k]].tobytes() != ref[k, :nref[k]].tobytes()
               for k in range(len(images)))
    assert dev.h.lib.vpk_lsd_set_math(dev.h.h, 2) == VPK_ERR_ARG
    assert dev.h.lib.vpk_lsd_set_math(dev.h.h, -1) == VPK_ERR_ARG
    assert dev.h.lib.vpk_lsd_set_math(None, 0) == VPK_ERR_ARG
