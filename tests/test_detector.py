"""The detector glue's device code (csrc/detect_device.hpp) compiled for the host by tests/hostsim/sim_detect.cpp and run
serially against NumPy -- the order of the best VPs is np.argsort(counts, kind="stable")[::-1][:maxbest] exactly, the pixel
conversion is the NumPy expression of example.py:66-76 byte for byte -- and the argument rules of detector.Detector and
example.py's --detector flag, checked without a GPU.  The kernels themselves: tests/test_gpu_detector.py, which imports
the tables below."""
import ctypes
import os

import numpy as np
import pytest

from hostsim import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))

V, I = ctypes.c_void_p, ctypes.c_int
ORDER_M = (0, 1, 2, 3, 15, 16, 17, 33, 63, 64)
ORDER_MAXBEST = (1, 3, 20, 64)
ORDER_KINDS = ("distinct", "equal", "three_values", "one_nan", "all_nan")
PIXEL_DIMS = ((640, 480), (427, 640), (1, 1), (1048576, 3))


def build_sim():
    lib = hostbuild.load("detect")
    lib.sim_vp_order.argtypes = [I, I, V, V, I, V]
    lib.sim_to_pixels.argtypes = [I, V, V, V, I] + [V] * 6
    return lib


@pytest.fixture(scope="module")
def sim():
    return build_sim()


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


# ---- order ----------------------------------------------------------------------------------------------------------
def stable_order(counts, maxbest):
    """The rule of include/vpk.h for one image: np.argsort(kind="stable")[::-1][:maxbest], zero padded to maxbest."""
    out = np.zeros(maxbest, dtype=np.int32)
    best = np.argsort(counts, kind="stable")[::-1][:maxbest]
    out[:best.size] = best
    return out


def order_counts(kind, m, rs):
    if kind == "distinct":
        return rs.permutation(m).astype(np.float64) + 3.0
    if kind == "equal":
        return np.full(m, 7.0)
    if kind == "three_values":
        return rs.choice([3.0, 4.0, 9.0], m)
    c = rs.choice([3.0, 4.0, 9.0, 11.0], m)
    if kind == "one_nan" and m:
        c[rs.randint(m)] = np.nan
    if kind == "all_nan":
        c[:] = np.nan
    return c


def order_table(max_vp=64):
    """(counts B x max_vp, num_vp B): every M of ORDER_M with every kind of counts; the entries past M hold large counts
    that a kernel ignoring num_vp would rank first."""
    rs = np.random.RandomState(11)
    rows, num = [], []
    for m in ORDER_M:
        for kind in ORDER_KINDS:
            row = np.full(max_vp, 1e6)
            row[:m] = order_counts(kind, m, rs)
            rows.append(row)
            num.append(m)
    return np.ascontiguousarray(rows), np.array(num, dtype=np.int32)


def order_want(counts, num, maxbest):
    return np.stack([stable_order(counts[b, :num[b]], maxbest) for b in range(len(num))])


def sim_order(sim, counts, num, maxbest):
    batch, max_vp = counts.shape
    out = np.full((batch, maxbest), -7, dtype=np.int32)
    assert sim.sim_vp_order(batch, max_vp, _p(counts), _p(num), maxbest, _p(out)) == 0
    return out


@pytest.mark.parametrize("maxbest", ORDER_MAXBEST)
def test_order_is_the_stable_argsort_reversed(sim, maxbest):
    counts, num = order_table()
    got = sim_order(sim, counts, num, maxbest)
    want = order_want(counts, num, maxbest)
    assert np.array_equal(got, want)
    for b, m in enumerate(num):                                  # the padding, said on its own
        assert (got[b, min(maxbest, m):] == 0).all()


def test_order_tie_rule_in_words(sim):
    """Among equal counts the higher index first; NaN above every number, among NaNs the higher index first."""
    c = np.array([[5.0, np.nan, 5.0, 9.0, np.nan, 5.0, 1.0, 0.0]])
    got = sim_order(sim, c, np.array([7], dtype=np.int32), 8)
    assert got.tolist() == [[4, 1, 3, 5, 2, 0, 6, 0]]
    # num_vp is clamped to 0..max_vp as horizon_kernel clamps it
    assert np.array_equal(sim_order(sim, c, np.array([-3], dtype=np.int32), 4), np.zeros((1, 4), np.int32))
    assert np.array_equal(sim_order(sim, c, np.array([99], dtype=np.int32), 8)[0], stable_order(c[0], 8))


# ---- pixels ---------------------------------------------------------------------------------------------------------
def numpy_point_px(x, y, w, h):
    """example.py:66-76 on arrays."""
    scale = max(w, h)
    return x * scale / 2.0 + w / 2.0, -y * scale / 2.0 + h / 2.0


def numpy_pixels(dims, offsets, lp, vp, num_vp, horizon):
    """(lp_px, vp_px, horizon_px) of vpk_to_pixels_batch from the NumPy expression."""
    batch, max_vp = vp.shape[0], vp.shape[1]
    lp_px = np.empty_like(lp)
    vp_px = np.full((batch, max_vp, 2), np.nan)
    hz_px = np.empty((batch, 2, 2))
    with np.errstate(all="ignore"):
        for b in range(batch):
            w, h = int(dims[b, 0]), int(dims[b, 1])
            s = lp[offsets[b]:offsets[b + 1]]
            o = lp_px[offsets[b]:offsets[b + 1]]
            o[:, 0], o[:, 1] = numpy_point_px(s[:, 0], s[:, 1], w, h)
            o[:, 2], o[:, 3] = numpy_point_px(s[:, 2], s[:, 3], w, h)
            m = min(max(int(num_vp[b]), 0), max_vp)
            v = vp[b, :m]
            vp_px[b, :m, 0], vp_px[b, :m, 1] = numpy_point_px(v[:, 0] / v[:, 2], v[:, 1] / v[:, 2], w, h)
            for e in range(2):
                p = horizon[b, 3 * e:3 * e + 3]
                hz_px[b, e] = numpy_point_px(p[0], p[1], w, h)
    return lp_px, vp_px, hz_px


def pixel_table(max_vp=8):
    """One image per entry of PIXEL_DIMS plus an image without segments and VPs: points 0, +-1, +-1e-300 and random; a VP
    with v[2] = 0 and one with all three components 0; num_vp below max_vp, so that NaN rows follow."""
    rs = np.random.RandomState(12)
    special = np.array([0.0, 1.0, -1.0, 1e-300, -1e-300, -0.0])
    dims = np.array(PIXEL_DIMS + ((33, 77),), dtype=np.int32)
    batch = dims.shape[0]
    n = [13, 6, 9, 21, 0]
    offsets = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    lp = rs.uniform(-1.2, 1.2, (int(offsets[-1]), 4))
    for b in range(batch):
        k = min(n[b], special.size)
        lp[offsets[b]:offsets[b] + k, 0] = special[:k]
        lp[offsets[b]:offsets[b] + k, 1] = special[:k][::-1]
        lp[offsets[b]:offsets[b] + k, 2] = np.roll(special, 2)[:k]
    vp = rs.normal(size=(batch, max_vp, 3))
    vp /= np.linalg.norm(vp, axis=2, keepdims=True)
    num_vp = np.array([6, 8, 5, 7, 0], dtype=np.int32)
    for b in range(batch - 1):
        vp[b, 0] = (0.6, 0.8, 0.0)                               # at infinity
        vp[b, 1] = (0.0, 0.0, 0.0)
        vp[b, 2] = (0.0, 0.0, 1.0)
        vp[b, 3] = (-0.0, 1.0, -0.0)
    horizon = rs.uniform(-2.0, 2.0, (batch, 15))
    horizon[0, :6] = (1.0, 0.0, 1.0, -1.0, 0.0, 1.0)             # the no-VP default (calc_horizon.py:212-217)
    horizon[1, :6] = (1.0, np.nan, 1.0, -1.0, np.inf, 1.0)
    return dims, offsets, np.ascontiguousarray(lp), np.ascontiguousarray(vp), num_vp, horizon


def sim_pixels(sim, dims, offsets, lp, vp, num_vp, horizon, want=(True, True, True)):
    batch, max_vp = vp.shape[0], vp.shape[1]
    outs = [np.full(s, -7.25) if w else None
            for s, w in zip((lp.shape, (batch, max_vp, 2), (batch, 2, 2)), want)]
    assert sim.sim_to_pixels(batch, _p(dims), _p(offsets), _p(lp), max_vp, _p(vp), _p(num_vp), _p(horizon),
                             _p(outs[0]), _p(outs[1]), _p(outs[2])) == 0
    return outs


def test_pixels_equal_numpy_byte_for_byte(sim):
    table = pixel_table()
    got = sim_pixels(sim, *table)
    want = numpy_pixels(*table)
    for name, g, w in zip(("lp_px", "vp_px", "horizon_px"), got, want):
        assert g.tobytes() == w.tobytes(), name
    dims, _, _, vp, num_vp, _ = table
    vp_px = got[1]
    for b in range(dims.shape[0]):
        assert np.isnan(vp_px[b, num_vp[b]:]).all()              # rows at or past num_vp
    assert np.isinf(vp_px[0, 0]).all() and np.isnan(vp_px[0, 1]).all()      # v[2] = 0; all three 0
    assert not np.isnan(got[0]).any()


@pytest.mark.parametrize("want", [(True, False, False), (False, True, False), (False, False, True), (False, False, False)])
def test_pixels_null_outputs(sim, want):
    table = pixel_table()
    full = sim_pixels(sim, *table)
    part = sim_pixels(sim, *table, want=want)
    for f, g, w in zip(full, part, want):
        assert (g is None) if not w else g.tobytes() == f.tobytes()


@pytest.mark.parametrize("w,h", PIXEL_DIMS[:2] + ((200, 200),))
def test_pixels_invert_the_front_ends_normalisation(sim, w, h):
    """Random pixel segments, normalised as frontend.detect_lsd_lines normalises a detector's rows (evaluation.py:240-249),
    come back to the pixels within 1e-9."""
    from vanishing_points_2017_amd import frontend
    rs = np.random.RandomState(13)
    px = rs.uniform(0, 1, (50, 4)) * [w, h, w, h]
    rows = np.concatenate([px, np.ones((50, 3))], axis=1)
    seg = np.ascontiguousarray(frontend.detect_lsd_lines(np.full((h, w), 128.0), detector=lambda image: rows)["segments"])
    assert np.abs(seg).max() <= 1.0
    dims = np.array([[w, h]], dtype=np.int32)
    off = np.array([0, 50], dtype=np.int64)
    got = sim_pixels(sim, dims, off, seg, np.zeros((1, 1, 3)), np.zeros(1, np.int32), np.zeros((1, 15)),
                     want=(True, False, False))[0]
    assert np.abs(got - px).max() <= 1e-9


# ---- surface --------------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_gpu(monkeypatch):
    from vanishing_points_2017_amd import detector, em, frontend, runtime

    def refuse(*a, **k):
        raise AssertionError("the GPU was touched")
    for mod in (detector, em, runtime):
        monkeypatch.setattr(mod, "get_runtime", refuse)
    monkeypatch.setattr(frontend, "lines_batch_device", refuse)
    return refuse


class _NoNet(object):
    def __getattr__(self, name):
        raise AssertionError("the net was touched (%s)" % name)


def test_bad_arguments_are_refused_before_the_gpu_is_touched(no_gpu):
    from vanishing_points_2017_amd.detector import Detector
    with pytest.raises(AssertionError, match="area"):
        Detector(_NoNet(), distance_measure="area")
    with pytest.raises(TypeError, match="no_such_keyword"):
        Detector(_NoNet(), no_such_keyword=3)
    with pytest.raises(ValueError, match="maxbest"):
        Detector(_NoNet(), maxbest=65)
    with pytest.raises(ValueError):
        Detector(_NoNet(), range_policy="sometimes")
    det = Detector(_NoNet(), distance_measure="dotprod", num_iter=7, maxbest=64)
    assert det.params.num_iter == 7 and det.distance_measure == "dotprod"
    ok = np.zeros((40, 30, 3), np.uint8)
    for bad in (np.zeros((40, 30), np.float64), np.zeros((40, 30, 4), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            det.detect_device([ok, bad])
        with pytest.raises(ValueError, match="uint8"):
            det.detect([bad])


def test_example_lists_the_detector_flag(capsys):
    from vanishing_points_2017_amd import example
    with pytest.raises(SystemExit) as e:
        example.main(["--help"])
    assert e.value.code == 0
    assert "--detector" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:                         # the flag belongs to --source_folder
        example.main(["--detector"])
    assert e.value.code == 2


def test_entry_points_are_declared_and_exported():
    from vanishing_points_2017_amd import _lib, calc_horizon
    assert {"vpk_vp_order_batch", "vpk_to_pixels_batch"} <= set(_lib.EXPORTS)
    assert callable(calc_horizon.vp_order_batch_device) and callable(calc_horizon.horizon_batch_device)
    text = open(os.path.join(HERE, "..", "include", "vpk.h")).read()
    assert "int vpk_vp_order_batch(" in text and "int vpk_to_pixels_batch(" in text
