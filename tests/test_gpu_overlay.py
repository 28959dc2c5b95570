"""vpk_overlay_lines_batch and vpk_overlay_markers_batch (csrc/vpk_overlay.hip) through the C-ABI, and result_plotting on
top of them, against the NumPy restatement of DESIGN section 7d: the cases, the rule and the cap of
tests/overlay_reference.py, the same as the host build's (tests/test_overlay.py).

Every launch blends into a buffer with guard bytes behind each image, the last one included; no guard byte may change."""
import ctypes

import numpy as np
import pytest

import overlay_reference as R

pytestmark = pytest.mark.gpu

VPK_ERR_ARG = -1
GUARD, FILL = 64, 0xA5


def _rt():
    from vanishing_points_2017_amd.runtime import get_runtime
    return get_runtime(0)


def _P():
    from vanishing_points_2017_amd import result_plotting
    return result_plotting


def _h(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def raw(disc, dims, pix, rgb, off, geom, rgba, width, batch=None):
    """The C entry: (return code, the byte buffer afterwards)."""
    rt = _rt()
    torch = rt.torch
    dims32 = np.ascontiguousarray(dims[:, 0] if disc else dims.reshape(-1), dtype=np.int32)
    pix, off = np.ascontiguousarray(pix, dtype=np.int64), np.ascontiguousarray(off, dtype=np.int64)
    fn = rt.lib.vpk_overlay_markers_batch if disc else rt.lib.vpk_overlay_lines_batch
    with rt.on_stream():
        d_rgb = torch.from_numpy(rgb.copy()).to(rt.tdev)
        d_geom, d_rgba, d_width = (torch.from_numpy(np.ascontiguousarray(a)).to(rt.tdev) for a in (geom, rgba, width))
        rc = fn(rt.h, len(pix) - 1 if batch is None else batch, _h(dims32), _h(pix), rt.ptr(d_rgb), _h(off), rt.ptr(d_geom),
                rt.ptr(d_rgba), rt.ptr(d_width))
    rt.synchronize()
    return rc, d_rgb.cpu().numpy()


@pytest.mark.parametrize("name", R.CASES)
def test_kernels_equal_the_reference(name):
    c = R.case(name)
    dims, pix, rgb, off, geom, rgba, width = R.flatten(c, GUARD, FILL)
    rc, out = raw(c['disc'], dims, pix, rgb, off, geom, rgba, width)
    assert rc == 0
    R.check_case(name, out, pix, GUARD, FILL)


def test_markers_entry_equals_zero_length_segments():
    """A disc is a segment without length: both entries give the same bytes."""
    c = R.case("discs")
    dims, pix, rgb, off, geom, rgba, width = R.flatten(c, GUARD, FILL)
    rc1, a = raw(True, dims, pix, rgb, off, geom, rgba, width)
    rc2, b = raw(False, dims, pix, rgb, off, np.concatenate([geom, geom], axis=1), rgba, width)
    assert rc1 == 0 and rc2 == 0 and np.array_equal(a, b)


def test_bad_arguments():
    c = R.case("ragged")
    dims, pix, rgb, off, geom, rgba, width = R.flatten(c, GUARD, FILL)

    def refused(**kw):
        args = dict(disc=False, dims=dims, pix=pix, rgb=rgb, off=off, geom=geom, rgba=rgba, width=width)
        args.update(kw)
        rc, out = raw(**args)
        assert rc == VPK_ERR_ARG and np.array_equal(out, rgb)          # nothing was launched
        assert b"vpk_overlay" in _rt().lib.vpk_last_error(_rt().h)

    refused(batch=-1)
    for bad in ([0, 33], [17, -1]):
        d = dims.copy()
        d[0] = bad
        refused(dims=d)
    refused(pix=pix[[0, 2, 1, 3]])                                     # offsets that do not rise
    p = pix.copy()
    p[1] -= GUARD + 1                                                  # image 0 would reach into image 1
    refused(pix=p)
    p = pix.copy()
    p[0] = -3
    refused(pix=p)
    refused(off=off[[0, 2, 1, 3]])
    d = dims.copy()
    d[:, 1] = d[:, 0]
    refused(disc=True, dims=-d, geom=geom[:, :2])
    rt = _rt()
    assert rt.lib.vpk_overlay_lines_batch(None, 1, None, None, None, None, None, None, None) == VPK_ERR_ARG
    assert raw(False, dims, pix, rgb, off, geom, rgba, width, batch=0)[0] == 0


def _scene_args():
    ds, ims, tv, hz = zip(*[R.golden_datum(n, w, h) for n, (w, h) in zip(R.GOLDEN_SCENES, ((64, 48), (33, 17), (40, 40)))])
    return list(ds), list(ims), list(tv), list(hz)


def test_batch_equals_one_by_one():
    P = _P()
    ds, ims, tv, hz = _scene_args()
    assert len({d['lines']['line_segments'].shape[0] for d in ds}) == 3
    batch = P.render_em_results_batch(ds, ims, maxbest=4, true_vps=tv, horizons=hz, cell=4)
    for d, im, t, h, got in zip(ds, ims, tv, hz, batch):
        one = P.render_em_result(d, im, maxbest=4, true_vps=t, horizon=h, cell=4)
        for key in ('image', 'sphere', 'response'):
            assert got[key].dtype == np.uint8 and got[key].shape[2] == 3
            assert np.array_equal(got[key], one[key]), key
        assert got['image'].shape == im.shape and got['sphere'].shape == (500, 500, 3) and got['response'].shape == (80, 80, 3)
        assert not np.array_equal(got['image'], im)


def test_panels_against_the_reference_renderer():
    """The three panels of one stored scene against the NumPy renderer on the layer's own draw lists."""
    P = _P()
    datum, image, true_vps, horizon = R.golden_datum("yud_n120")
    out = P.render_em_result(datum, image, maxbest=3, true_vps=true_vps, horizon=horizon, cell=4)
    h, w = image.shape[:2]
    p = P.segments_to_pixels([[horizon[0][0], horizon[0][1], horizon[1][0], horizon[1][1]]], w, h)[0]
    R.check(out['image'], R.render(image, *P.line_primitives(datum, w, h, 3, ((p[0], p[1]), (p[2], p[3])))))
    R.check(out['response'], R.render(P.response_panel(datum['cnn_prediction'], 4), *P._result_markers(datum, 20, 4, 3, true_vps)))
    R.check(out['sphere'], R.render(P.to_rgb(datum['sphere_image']), *P._result_markers(datum, 500, 1, 3, true_vps)))
    part = {k: v for k, v in datum.items() if k != 'cnn_prediction'}
    o2 = P.render_em_result(part, image)
    assert o2['response'] is None and o2['sphere'] is not None
    with pytest.raises(AssertionError):
        P.render_em_result({k: v for k, v in datum.items() if k != 'lines'}, image)


def test_show_em_result_writes_the_image_panel(tmp_path):
    from PIL import Image
    P = _P()
    datum, image, _, _ = R.golden_datum("tiny_n12")
    src, dst = str(tmp_path / "scene.png"), str(tmp_path / "overlay.png")
    Image.fromarray(image).save(src)
    out = P.show_em_result(datum, src, maxbest=2, horizon=((2.0, 30.0), (60.0, 28.0)), out_file=dst)
    assert np.array_equal(np.asarray(Image.open(dst)), out['image'])
    h, w = image.shape[:2]
    R.check(out['image'], R.render(image, *P.line_primitives(datum, w, h, 2, ((2.0, 30.0), (60.0, 28.0)))))
    small = P.show_em_result(datum, src, target_size=32)
    assert small['image'].shape == (24, 32, 3)


def test_save_overlays_writes_one_file_per_image(tmp_path):
    """example.py --save-overlays for the images of a folder: an image with VPs gets its lines and horizon, an image
    without VPs its plain (resized) image -- one file each."""
    from PIL import Image
    from vanishing_points_2017_amd import example, frontend
    P = _P()
    datum, image, _, _ = R.golden_datum("tiny_n12", 80, 60)
    src = str(tmp_path / "scene.png")
    Image.fromarray(image).save(src)
    out = str(tmp_path / "overlays")
    hz = ((2.0, 300.0), (630.0, 280.0))
    f1 = example.save_file_overlay(out, src, datum, hz)
    big = frontend.resize_to_fit(image, 640)
    assert big.shape == (480, 640, 3)
    got = np.asarray(Image.open(f1))
    R.check(got, R.render(big, *P.line_primitives(datum, 640, 480, 4, hz)))
    assert not np.array_equal(got, big)
    none = dict(datum, EM_result={'vp': None, 'counts': None, 'vp_assoc': None})
    src2 = str(tmp_path / "empty.png")
    Image.fromarray(image).save(src2)
    f2 = example.save_file_overlay(out, src2, none, None)
    assert f1 != f2 and np.array_equal(np.asarray(Image.open(f2)), big)
    assert sorted(p.name for p in (tmp_path / "overlays").iterdir()) == ["empty_overlay.png", "scene_overlay.png"]


def test_example_save_overlays_flag(tmp_path, capsys):
    """The flag itself, on the synthetic scene: one PNG of the scene's size with lines drawn on black."""
    from PIL import Image
    from vanishing_points_2017_amd import example
    example.main(["--save-overlays", str(tmp_path), "--lines", "150", "--seed", "7"])
    assert "overlay:" in capsys.readouterr().out
    files = list(tmp_path.iterdir())
    assert [f.name for f in files] == ["synthetic_seed7_overlay.png"]
    a = np.asarray(Image.open(str(files[0])))
    assert a.ndim == 3 and a.shape[2] == 3 and a.shape[1] == 640 and a.any() and (a == 0).all(axis=2).mean() > 0.5
