"""The overlay renderer's device code (csrc/overlay_device.hpp) compiled for the host by tests/hostsim/sim_overlay.cpp and run
serially, against the NumPy restatement of DESIGN section 7d (tests/overlay_reference.py: the rule, the cap and the cases),
and result_plotting's Python layer -- draw lists, best-VP order, panels -- without a GPU (where it needs pixels, the host
build stands in for the kernels).  The kernels themselves: tests/test_gpu_overlay.py."""
import ctypes

import numpy as np
import pytest

import overlay_reference as R
from hostsim import hostbuild

GUARD, FILL = 64, 0xA5


def _sim():
    lib = hostbuild.load("overlay")
    lib.sim_overlay.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 7
    return lib


@pytest.fixture(scope="module")
def sim():
    return _sim()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_sim(lib, disc, dims, pix, rgb, off, geom, rgba, width):
    rgb = rgb.copy()
    keep = [np.ascontiguousarray(a) for a in (dims.astype(np.int64), pix, off, geom, rgba, width)]
    assert lib.sim_overlay(int(disc), len(pix) - 1, _p(keep[0]), _p(keep[1]), _p(rgb), _p(keep[2]), _p(keep[3]), _p(keep[4]),
                           _p(keep[5])) == 0
    return rgb


@pytest.mark.parametrize("name", R.CASES)
def test_host_build_equals_the_reference(sim, name):
    c = R.case(name)
    dims, pix, rgb, off, geom, rgba, width = R.flatten(c, GUARD, FILL)
    before = [a.copy() for a in (geom, rgba, width)]
    out = run_sim(sim, c['disc'], dims, pix, rgb, off, geom, rgba, width)
    R.check_case(name, out, pix, GUARD, FILL)
    assert all(np.array_equal(a, b) for a, b in zip((geom, rgba, width), before))


def test_primitives_that_are_not_finite_are_not_drawn(sim):
    c = R._one(40, 23, [[np.nan, 3, 20, 9], [4, 5, np.inf, 9], [4, 5, 20, 9], [4, 5, 20, 9], [3, 12, 30, 14]],
               [R.RED] * 5, [3, 3, np.nan, -1, 3])
    ref = R.render(c['images'][0], *c['prims'][0])
    only = R.render(c['images'][0], c['prims'][0][0][4:], c['prims'][0][1][4:], c['prims'][0][2][4:])
    assert np.array_equal(ref['rgb'], only['rgb']) and ref['drawn'].any()
    dims, pix, rgb, off, geom, rgba, width = R.flatten(c)
    out = run_sim(sim, False, dims, pix, rgb, off, geom, rgba, width)
    R.check(out.reshape(c['images'][0].shape), ref)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def _P():
    from vanishing_points_2017_amd import result_plotting
    return result_plotting


def test_best_vp_order_and_colours():
    P = _P()
    assert list(P.best_vps([3, 5, 5, 1, 5], 3)) == [1, 2, 4]           # equal counts: by index
    assert list(P.best_vps([3, 5, 5, 1, 5], 4)) == [1, 2, 4, 0]
    assert list(P.best_vps([2.0, 7.0], 4)) == [1, 0]                   # maxbest beyond the number of VPs
    assert P.best_colours(0).shape == (0, 3)
    assert P.best_colours(1).tolist() == [[0, 0, 128]]                 # t = 0: r = g = 0, b = clip(1.5 - 1) = 0.5 -> 128
    assert P.best_colours(3).tolist() == [[0, 0, 128], [128, 255, 128], [128, 0, 0]]
    t = 1.0 / 3.0                                                      # the second of four, by the formulas of DESIGN 7d
    want = [int(np.floor(255 * np.clip(1.5 - abs(4 * t - s), 0, 1) + 0.5)) for s in (3, 2, 1)]
    assert P.best_colours(4)[1].tolist() == want


@pytest.mark.parametrize("name", R.GOLDEN_SCENES)
def test_line_list_equals_the_reference_loop(name):
    """The draw list against a restatement of result_plotting.py:56-59 and :94-97 on a stored EM result."""
    P = _P()
    datum, image, _, horizon = R.golden_datum(name)
    h, w = image.shape[:2]
    ls, res = datum['lines']['line_segments'], datum['EM_result']
    maxbest = 4
    scale = np.maximum(w, h)
    lsc = ls.copy()
    lsc[:, 0] = lsc[:, 0] * scale / 2.0 + w / 2.0
    lsc[:, 2] = lsc[:, 2] * scale / 2.0 + w / 2.0
    lsc[:, 1] = -lsc[:, 1] * scale / 2.0 + h / 2.0
    lsc[:, 3] = -lsc[:, 3] * scale / 2.0 + h / 2.0
    best = P.best_vps(res['counts'], maxbest)
    assert sorted(res['counts'][best], reverse=True) == list(res['counts'][best])
    assert set(res['counts'][best]) == set(np.sort(res['counts'])[::-1][:maxbest])
    colours = P.best_colours(best.size)
    want_seg, want_col = [], []
    for li in range(ls.shape[0]):
        if res['vp_assoc'][li] in best:
            idx_best = int(np.squeeze(np.where(best == res['vp_assoc'][li])[0]))
            want_seg.append(lsc[li])
            want_col.append(list(colours[idx_best]) + [255])
    hz_px = ((1.5, 20.25), (60.0, 22.5))
    seg, rgba, width = P.line_primitives(datum, w, h, maxbest, hz_px)
    assert len(want_seg) > 0
    assert np.array_equal(seg[:-1], np.array(want_seg)) and np.array_equal(rgba[:-1], np.array(want_col, dtype=np.uint8))
    assert (width[:-1] == 2).all()
    assert seg[-1].tolist() == [1.5, 20.25, 60.0, 22.5] and rgba[-1].tolist() == [0, 255, 255, 255] and width[-1] == 10
    assert np.array_equal(ls, R.golden_datum(name)[0]['lines']['line_segments'])
    # maxbest beyond the number of VPs: every assigned line is drawn
    seg_all, _, _ = P.line_primitives(datum, w, h, 1000)
    assert seg_all.shape[0] == int((res['vp_assoc'] >= 0).sum())


def test_unassigned_lines_are_not_drawn():
    P = _P()
    datum = {'lines': {'line_segments': np.array([[0.0, 0, 0.5, 0.5], [0.1, 0.2, 0.3, 0.4], [-0.5, 0, 0.5, 0], [0, 0, 0.1, 0.1]])},
             'EM_result': {'vp': np.eye(3), 'counts': np.array([1.0, 2.0, 1.0]), 'vp_assoc': np.array([-1, 1, 0, 2])}}
    seg, rgba, width = P.line_primitives(datum, 40, 20, maxbest=2)
    # best = [1, 0]: line 1 takes the first colour, line 2 the second; line 0 has no VP and line 3's VP is not among the best
    assert seg.tolist() == [[22.0, 6.0, 26.0, 2.0], [10.0, 10.0, 30.0, 10.0]]
    assert rgba.tolist() == [[0, 0, 128, 255], [128, 0, 0, 255]] and width.tolist() == [2.0, 2.0]
    assert P.line_primitives(dict(datum, EM_result=None), 40, 20)[0].shape == (0, 4)


def test_marker_list():
    P = _P()
    from vanishing_points_2017_amd import coordinate_conversion as cc, probability_functions as prob
    vps = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 0.6, 0.8]])
    ang = prob.calc_angles(3, vps)
    counts = np.array([90.0, 9.0, 1.0])
    xy, rgba, diam = P.marker_primitives(vps, ang, counts, best=[0], img_size=20, cell=10)
    for j in range(3):
        pos = cc.angle_to_index(ang[j], (20, 20))
        assert xy[j].tolist() == [pos[0] * 10.0, (20 - 1 - pos[1]) * 10.0]
    assert np.array_equal(cc.angles_to_indices(ang, (20, 20)), np.stack([cc.angle_to_index(a, (20, 20)) for a in ang]))
    assert diam.tolist() == [200.0, 90.0, 60.0]                        # min(max(100 share, 6), 20) x cell
    assert rgba.tolist() == [[0, 128, 0, 153], [191, 191, 0, 153], [191, 191, 0, 153]]
    _, rgba_c, diam_c = P.marker_primitives(vps, ang, None, None, img_size=250, std_mark='co')
    assert rgba_c.tolist() == [[0, 191, 191, 153]] * 3 and diam_c.tolist() == [6.0] * 3
    assert P.marker_primitives(vps, ang, None, None, std_mark='go')[1][0].tolist() == [0, 128, 0, 153]
    with pytest.raises(ValueError):
        P.marker_primitives(vps, ang, None, None, std_mark='rx')


def test_response_panel():
    P = _P()
    m = np.zeros((20, 20), np.float32)
    assert not P.response_panel(m, 3).any() and P.response_panel(m, 3).shape == (60, 60, 3)
    m[0, 1], m[19, 0] = 2.0, 0.5
    p = P.response_panel(m, 2)
    assert p.dtype == np.uint8 and p.shape == (40, 40, 3)
    assert (p[38:40, 2:4] == 255).all() and (p[0:2, 0:2] == 64).all()  # flipped vertically; floor(255 * 0.25 + 0.5) = 64
    assert int(p.astype(np.int64).sum()) == 3 * 4 * (255 + 64)


def test_missing_lines_raise_like_the_reference():
    P = _P()
    datum, image, _, _ = R.golden_datum("tiny_n12")
    bad = {k: v for k, v in datum.items() if k != 'lines'}
    with pytest.raises(AssertionError):
        P.render_em_result(bad, image)
    with pytest.raises(AssertionError):
        P.render_em_results_batch([bad], [image])


@pytest.fixture()
def host_kernels(sim, monkeypatch):
    """result_plotting.overlay_batch with the host build in place of the two kernels."""
    P = _P()

    def overlay_batch(panels, prims, discs, device=0):
        if not panels:
            return []
        c = {'disc': discs, 'images': panels, 'prims': prims}
        dims, pix, rgb, off, geom, rgba, width = R.flatten(c)
        out = run_sim(sim, discs, dims, pix, rgb, off, geom, rgba, width)
        return [out[pix[b]:pix[b + 1]].reshape(p.shape).copy() for b, p in enumerate(panels)]

    monkeypatch.setattr(P, "overlay_batch", overlay_batch)
    return P


def test_panels_on_a_stored_scene(host_kernels):
    """The three panels of one stored scene through the Python layer, each against the reference renderer on the layer's own
    draw lists; panels whose source is missing are None."""
    P = host_kernels
    datum, image, true_vps, horizon = R.golden_datum("tiny_n12")
    out = P.render_em_result(datum, image, maxbest=4, true_vps=true_vps, horizon=horizon, cell=3)
    assert set(out) == {'image', 'sphere', 'response'}
    h, w = image.shape[:2]
    hz = P.segments_to_pixels([[horizon[0][0], horizon[0][1], horizon[1][0], horizon[1][1]]], w, h)[0]
    lines = P.line_primitives(datum, w, h, 4, ((hz[0], hz[1]), (hz[2], hz[3])))
    R.check(out['image'], R.render(image, *lines))
    assert lines[1][-1].tolist() == [0, 255, 255, 255] and not np.array_equal(out['image'], image)
    marks = P._result_markers(datum, 20, 3, 4, true_vps)
    assert marks[2].size == datum['EM_result']['vp'].shape[0] + true_vps.shape[0]
    assert (marks[1][-true_vps.shape[0]:, :3] == (0, 191, 191)).all() and (marks[2][-true_vps.shape[0]:] == 18).all()
    assert out['response'].shape == (60, 60, 3)
    R.check(out['response'], R.render(P.response_panel(datum['cnn_prediction'], 3), *marks))
    assert out['sphere'].shape == (500, 500, 3)
    grey = P.to_rgb(datum['sphere_image'])
    untouched = out['sphere'] == grey
    assert not untouched.all() and untouched.mean() > 0.9
    # panels without a source are None; a datum without an EM result gets unmarked panels
    part = {k: v for k, v in datum.items() if k not in ('sphere_image', 'cnn_prediction')}
    o2 = P.render_em_result(part, image)
    assert o2['sphere'] is None and o2['response'] is None and o2['image'].shape == image.shape
    o3 = P.render_em_result(dict(datum, EM_result=None), image[:, :, 0])
    assert np.array_equal(o3['image'], P.to_rgb(image[:, :, 0])) and np.array_equal(o3['sphere'], grey)
    # plot_result on a prepared panel is the same marker pass
    from vanishing_points_2017_amd import probability_functions as prob
    res = datum['EM_result']
    one = P.plot_result(P.response_panel(datum['cnn_prediction'], 3), res['vp'], prob.calc_angles(res['vp'].shape[0], res['vp']),
                        res['counts'], P.best_vps(res['counts'], 4), img_size=20)
    both = P.render_em_result(datum, image, cell=3)
    assert np.array_equal(one, both['response'])
