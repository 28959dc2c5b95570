"""coordinate_conversion against values captured from the reference (tests/golden/plotting/coconv.npz, written by
scripts/make_plotting_golden.py): equal to the last bit on the shapes (20, 20), (500, 500) and (250, 500); angles 0, +-pi/2
and 1000 seeded ones; points with point[2] < 0 and point[2] == 0; the round trip within 1e-12."""
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "plotting", "coconv.npz"), allow_pickle=False))


def _cc():
    from vanishing_points_2017_amd import coordinate_conversion
    return coordinate_conversion


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_the_captured_inputs_are_the_ones_asked_for(g):
    assert g['shapes'].tolist() == [[20, 20], [500, 500], [250, 500]]
    h = np.pi / 2
    assert g['angles'].shape == (1009, 2) and g['angles'][0].tolist() == [0.0, 0.0]
    assert {tuple(a) for a in g['angles'][:9].tolist()} == {(a, b) for a in (0.0, -h, h) for b in (0.0, -h, h)}
    assert (g['points'][:, 2] < 0).sum() >= 100 and (g['points'][:, 2] == 0).sum() >= 4
    assert float(g['sign0']) == 0.0 == float(np.sign(0.0))


def test_angle_to_index_bit_for_bit(g):
    cc = _cc()
    for s, want in zip(g['shapes'], g['angle_to_index']):
        shape = tuple(int(v) for v in s)
        got = np.stack([cc.angle_to_index(a, shape) for a in g['angles']])
        assert _same(got, want)
        assert _same(cc.angles_to_indices(g['angles'], shape), want)
    assert isinstance(cc.angle_to_index(g['angles'][3], (20, 20)), np.ndarray)
    assert cc.angles_to_indices(np.zeros((0, 2)), (20, 20)).shape == (0, 2)


def test_index_to_angle_bit_for_bit(g):
    cc = _cc()
    for s, idx, want in zip(g['shapes'], g['indices'], g['index_to_angle']):
        shape = tuple(int(v) for v in s)
        assert _same(np.stack([cc.index_to_angle(i, shape) for i in idx]), want)


def test_angle_to_point_bit_for_bit(g):
    cc = _cc()
    got = np.stack([cc.angle_to_point(a) for a in g['point_angles']])
    assert _same(got, g['angle_to_point'])
    flipped = np.cos(g['point_angles'][:, 0]) * np.cos(g['point_angles'][:, 1]) < 0         # :48 changed the sign
    assert flipped.sum() >= 12 and (got[flipped, 2] > 0).all()


def test_point_to_angle_bit_for_bit(g):
    cc = _cc()
    with np.errstate(all="ignore"):
        got = np.stack([cc.point_to_angle(p) for p in g['points']])
    assert _same(got, g['point_to_angle'])
    clamped = np.abs(g['points'][:, 0] / np.cos(np.arcsin(g['points'][:, 1]))) > 1              # :57-58
    assert clamped.any() and np.allclose(np.abs(got[clamped, 0]), np.pi / 2)
    zero = g['points'][:, 2] == 0
    assert zero.sum() >= 4 and np.isfinite(got[zero]).all()


def test_sign_of_zero_gives_the_zero_vector():
    """No float64 angle has a cosine of exactly 0, so angle_to_point cannot produce point[2] == 0 from finite angles; what
    :48 does there is NumPy's sign(0) = 0, shown on the multiplication itself."""
    p = np.array([0.5, 0.5, 0.0])
    p *= np.sign(p[2])
    assert p.tolist() == [0.0, 0.0, 0.0]
    cc = _cc()
    assert cc.angle_to_point(np.array([np.pi / 2, 0.3]))[2] > 0 and cc.angle_to_point(np.array([-np.pi / 2, 0.3]))[2] > 0


def test_round_trip(g):
    cc = _cc()
    for s, idx in zip(g['shapes'], g['indices']):
        shape = tuple(int(v) for v in s)
        for i in idx:
            assert np.abs(cc.angle_to_index(cc.index_to_angle(i, shape), shape) - i).max() <= 1e-12
