"""The reference's result_plotting.py as headless overlays: the image with its lines coloured by vanishing point and the
horizon, and the CNN's input and output with the VPs marked -- uint8 RGB arrays for a whole batch, one kernel launch per
panel kind (csrc/vpk_overlay.hip), nothing displayed.

The reference draws through matplotlib's figure layout, which has no pixel-level definition; the renderer here is specified
in DESIGN section 7d and keeps the reference's CONTENT: which lines, which colours, which markers, what order.  The host
prepares the per-image primitive lists (pixel coordinates, colours, widths, in draw order: O(N) bookkeeping, the functions
``line_primitives`` and ``marker_primitives``); the per-pixel work is the kernels'.  There is no host renderer in the
package: without a GPU the render calls raise.  Citations are file:line of the reference's result_plotting.py."""
import ctypes

import numpy as np

from . import coordinate_conversion as coconv
from . import probability_functions as prob
from .ragged import offsets_of

CYAN_LINE = (0, 255, 255)                                        # c='c' on the image (:107)
MARK_RGB = {'y': (191, 191, 0), 'g': (0, 128, 0), 'c': (0, 191, 191)}   # matplotlib's single-letter colours 'y', 'g', 'c'
MARK_ALPHA = 153                                                 # alpha = 0.6 (:139) in 1/255ths: 153 / 255 == 0.6 in float64
LINE_WIDTH, HORIZON_WIDTH = 2.0, 10.0                            # lw=2 (:97), lw=10 (:107)
TRUE_VP_DIAMETER = 6.0


def best_vps(counts, maxbest):
    """np.argsort(counts)[::-1][:maxbest] (:73-75) with the package's tie order: descending count, ascending index among
    equal counts (NumPy's own order among equal counts belongs to its build)."""
    counts = np.asarray(counts, dtype=np.float64)
    return np.argsort(-counts, kind="stable")[:max(int(maxbest), 0)]


def best_colours(nbest):
    """The colour of the k-th best of ``nbest`` VPs (:85-87, :96): the piecewise-linear jet approximation at
    t = k / max(nbest - 1, 1), each channel stored as floor(255 c + 0.5).  Not matplotlib's table."""
    t = np.arange(nbest, dtype=np.float64) / max(nbest - 1, 1)
    rgb = np.stack([np.clip(1.5 - np.abs(4 * t - 3), 0, 1), np.clip(1.5 - np.abs(4 * t - 2), 0, 1),
                    np.clip(1.5 - np.abs(4 * t - 1), 0, 1)], axis=1)
    return np.floor(255 * rgb + 0.5).astype(np.uint8).reshape(nbest, 3)


def segments_to_pixels(ls, width, height):
    """Normalised end points -> pixel coordinates (:55-59): scale = max(W, H), y pointing down."""
    scale = np.maximum(width, height)
    lsc = np.array(ls, dtype=np.float64).reshape(-1, 4)
    lsc[:, 0] = lsc[:, 0] * scale / 2.0 + width / 2.0
    lsc[:, 2] = lsc[:, 2] * scale / 2.0 + width / 2.0
    lsc[:, 1] = -lsc[:, 1] * scale / 2.0 + height / 2.0
    lsc[:, 3] = -lsc[:, 3] * scale / 2.0 + height / 2.0
    return lsc


def _prims(geom, rgba, width, cols):
    return (np.ascontiguousarray(geom, dtype=np.float64).reshape(-1, cols),
            np.ascontiguousarray(rgba, dtype=np.uint8).reshape(-1, 4), np.ascontiguousarray(width, dtype=np.float64).reshape(-1))


def line_primitives(datum, width, height, maxbest=4, horizon_px=None):
    """The image panel's draw list (:53-107): (seg_px (P, 4), rgba (P, 4), width (P,)).  Every line whose vp_assoc is one
    of the best VPs, in line index order, in that VP's colour (lines of no VP, -1, or of a VP outside the best set are
    not drawn); then the horizon, two end points in pixel coordinates, in cyan.  The counts and vp_assoc of
    vp_localisation.calc_vp_line_counts, for any line set and VPs of the caller's, are an EM_result for this."""
    if datum.get('lines') is None:                               # :60-61 (raised, not asserted: python -O keeps it)
        raise AssertionError("the datum has no 'lines'")
    em_result = datum.get('EM_result')
    seg, rgba, wid = [], [], []
    if em_result is not None and em_result.get('vp') is not None:
        lsc = segments_to_pixels(datum['lines']['line_segments'], width, height)
        best = best_vps(em_result['counts'], maxbest)
        colours = best_colours(best.size)
        rank = np.full(max(int(np.asarray(em_result['counts']).size), 1), -1, dtype=np.int64)
        rank[best] = np.arange(best.size)
        assoc = np.asarray(em_result['vp_assoc']).astype(np.int64).reshape(-1)
        in_range = (assoc >= 0) & (assoc < rank.size)
        k = np.where(in_range, rank[np.where(in_range, assoc, 0)], -1)       # idx_best (:95), -1: not drawn (:94)
        drawn = np.nonzero(k >= 0)[0]
        seg.append(lsc[drawn])
        rgba.append(np.concatenate([colours[k[drawn]], np.full((drawn.size, 1), 255, np.uint8)], axis=1))
        wid.append(np.full(drawn.size, LINE_WIDTH))
        if horizon_px is not None:                               # :106-107
            seg.append(np.array([[horizon_px[0][0], horizon_px[0][1], horizon_px[1][0], horizon_px[1][1]]], dtype=np.float64))
            rgba.append(np.array([CYAN_LINE + (255,)], dtype=np.uint8))
            wid.append(np.array([HORIZON_WIDTH]))
    if not seg:
        return _prims(np.zeros((0, 4)), np.zeros((0, 4), np.uint8), np.zeros(0), 4)
    return _prims(np.concatenate(seg), np.concatenate(rgba), np.concatenate(wid), 4)


def marker_primitives(vps, angles, vp_counts, best=None, img_size=250, std_mark='yo', cell=1):
    """One square panel's markers (:113-139): (xy (P, 2), rgba (P, 4), diameter (P,)), VP index order.  VP j sits at
    pos = angle_to_index(angles[j], (img_size, img_size)), drawn at (pos[0], img_size - 1 - pos[1]) (:137-138); green if j
    is one of ``best``, else the colour of ``std_mark`` ('yo', 'go' or 'co'); opacity 0.6; diameter
    min(max(100 counts[j] / sum(counts), 6), 20) (:116, :139), 6 without counts.  On a panel whose cells are ``cell`` pixels
    wide, positions and diameters scale by ``cell``."""
    if std_mark not in ('yo', 'go', 'co'):
        raise ValueError("std_mark %r: the reference's markers are 'yo', 'go' and 'co'" % (std_mark,))
    m = int(np.asarray(vps).shape[0])
    if m == 0:
        return _prims(np.zeros((0, 2)), np.zeros((0, 4), np.uint8), np.zeros(0), 2)
    pos = coconv.angles_to_indices(np.asarray(angles, dtype=np.float64)[:m], (img_size, img_size))
    xy = np.stack([pos[:, 0], img_size - 1 - pos[:, 1]], axis=1) * float(cell)
    if vp_counts is not None:
        with np.errstate(all="ignore"):
            pg = np.asarray(vp_counts, dtype=np.float64)[:m] * 1.0 / np.sum(vp_counts)
            diam = np.minimum(np.maximum(pg * 100, 6), 20)
    else:
        diam = np.full(m, TRUE_VP_DIAMETER)
    rgba = np.empty((m, 4), dtype=np.uint8)
    rgba[:, :3] = MARK_RGB[std_mark[0]]
    if best is not None:
        rgba[np.asarray(best, dtype=np.int64).reshape(-1), :3] = MARK_RGB['g']     # :128-130
    rgba[:, 3] = MARK_ALPHA
    return _prims(xy, rgba, diam * float(cell), 2)


def _result_markers(datum, size, cell, maxbest, true_vps):
    """Markers of one panel of ``size`` cells: the result's VPs (:77-78), then the true VPs in cyan (:80-83)."""
    parts = []
    em_result = datum.get('EM_result')
    if em_result is not None and em_result.get('vp') is not None:
        vps = np.asarray(em_result['vp'], dtype=np.float64)
        parts.append(marker_primitives(vps, prob.calc_angles(vps.shape[0], vps), em_result['counts'],
                                       best_vps(em_result['counts'], maxbest), img_size=size, cell=cell))
        if true_vps is not None:
            tv = np.asarray(true_vps, dtype=np.float64).reshape(-1, 3)
            parts.append(marker_primitives(tv, prob.calc_angles(tv.shape[0], tv), None, None, img_size=size, std_mark='co',
                                           cell=cell))
    if not parts:
        return _prims(np.zeros((0, 2)), np.zeros((0, 4), np.uint8), np.zeros(0), 2)
    return _prims(*[np.concatenate([p[q] for p in parts]) for q in range(3)], cols=2)


def to_rgb(image):
    """uint8 H x W x 3 from a grey or colour uint8 image (a grey one is replicated; further channels are dropped)."""
    image = np.asarray(image)
    if image.dtype != np.uint8:
        raise TypeError("the panels are 8-bit images (got %s)" % image.dtype)
    if image.ndim == 2:
        return np.repeat(image[:, :, None], 3, axis=2)
    if image.ndim == 3 and image.shape[2] >= 3:
        return np.ascontiguousarray(image[:, :, :3])
    if image.ndim == 3 and image.shape[2] == 1:
        return np.repeat(image, 3, axis=2)
    raise ValueError("an image is H x W or H x W x 3 (got shape %s)" % (image.shape,))


def response_panel(cnn_prediction, cell=10):
    """The response map as a grey RGB panel: flipped vertically (:27), scaled to uint8 by its own maximum as
    floor(255 v / max + 0.5) (values below 0 count as 0; a map of zeros stays black), each cell ``cell`` x ``cell`` pixels."""
    p = np.asarray(cnn_prediction, dtype=np.float64)[::-1, :]
    top = p.max() if p.size else 0.0
    g = np.floor(255 * np.clip(p, 0, None) / top + 0.5).astype(np.uint8) if top > 0 else np.zeros(p.shape, np.uint8)
    return to_rgb(np.repeat(np.repeat(g, cell, axis=0), cell, axis=1))


def overlay_batch(panels, prims, discs, device=0):
    """Blend ``prims[b]`` (a draw list of line_primitives / marker_primitives) into ``panels[b]`` (uint8 H x W x 3) for
    every b in ONE launch; returns the new panels.  ``discs``: marker lists on square panels."""
    from .runtime import get_runtime
    rt = get_runtime(device)
    torch = rt.torch
    if not panels:
        return []
    panels = [np.ascontiguousarray(p, dtype=np.uint8) for p in panels]
    for p in panels:
        if p.ndim != 3 or p.shape[2] != 3 or (discs and p.shape[0] != p.shape[1]):
            raise ValueError("a panel is H x W x 3%s (got %s)" % (", square for markers" if discs else "", p.shape,))
    pix = offsets_of([p.size for p in panels])
    off = offsets_of([pr[2].size for pr in prims])
    cols = 2 if discs else 4
    geom = np.concatenate([pr[0].reshape(-1, cols) for pr in prims])
    rgba = np.concatenate([pr[1].reshape(-1, 4) for pr in prims])
    wid = np.concatenate([pr[2] for pr in prims])
    if discs:
        dims = np.array([p.shape[0] for p in panels], dtype=np.int32)
    else:
        dims = np.array([[p.shape[1], p.shape[0]] for p in panels], dtype=np.int32).reshape(-1)
    host = np.concatenate([p.reshape(-1) for p in panels])
    vp = ctypes.c_void_p
    with rt.on_stream():
        d_rgb = torch.from_numpy(host).to(rt.tdev)
        d_geom = torch.from_numpy(np.ascontiguousarray(geom)).to(rt.tdev)
        d_rgba = torch.from_numpy(np.ascontiguousarray(rgba)).to(rt.tdev)
        d_wid = torch.from_numpy(np.ascontiguousarray(wid)).to(rt.tdev)
        fn = rt.lib.vpk_overlay_markers_batch if discs else rt.lib.vpk_overlay_lines_batch
        rt.check(fn(rt.h, len(panels), dims.ctypes.data_as(vp), pix.ctypes.data_as(vp), rt.ptr(d_rgb), off.ctypes.data_as(vp),
                    rt.ptr(d_geom), rt.ptr(d_rgba), rt.ptr(d_wid)))
        out = d_rgb.cpu().numpy()
    rt.synchronize()
    return [out[pix[b]:pix[b + 1]].reshape(panels[b].shape).copy() for b in range(len(panels))]


def _render(datums, images, maxbest, true_vps, horizons_px, device, cell):
    datums, images = list(datums), list(images)
    if len(datums) != len(images):
        raise ValueError("%d datums but %d images" % (len(datums), len(images)))
    n = len(datums)
    true_vps = [None] * n if true_vps is None else list(true_vps)
    horizons_px = [None] * n if horizons_px is None else list(horizons_px)
    out = [{'image': None, 'sphere': None, 'response': None} for _ in range(n)]
    panels, prims = [], []
    for d, im, hz in zip(datums, images, horizons_px):
        rgb = to_rgb(im)
        panels.append(rgb)
        prims.append(line_primitives(d, rgb.shape[1], rgb.shape[0], maxbest, hz))
    for o, p in zip(out, overlay_batch(panels, prims, False, device)):
        o['image'] = p
    for key, source, c in (('sphere', 'sphere_image', 1), ('response', 'cnn_prediction', int(cell))):
        idx = [b for b in range(n) if datums[b].get(source) is not None]         # a missing panel stays None (:45-51)
        panels, prims = [], []
        for b in idx:
            src = datums[b][source]
            panels.append(to_rgb(src) if key == 'sphere' else response_panel(src, c))
            prims.append(_result_markers(datums[b], int(np.asarray(src).shape[0]), c, maxbest, true_vps[b]))
        for b, p in zip(idx, overlay_batch(panels, prims, True, device)):
            out[b][key] = p
    return out


def render_em_results_batch(datums, images, maxbest=4, true_vps=None, horizons=None, device=0, cell=10):
    """show_em_result's three panels (:11-110) for many results: per datum a dict with the uint8 RGB arrays 'image'
    (H x W x 3: the lines of the ``maxbest`` best VPs coloured by VP, then the horizon), 'sphere' (the CNN's input with
    the VPs marked) and 'response' (the CNN's output, each cell ``cell`` pixels wide, likewise); one launch per panel
    kind for the whole batch.
      datums    the dicts run_em writes: 'lines', 'sphere_image', 'cnn_prediction', 'EM_result'.  Without 'lines':
                AssertionError (:61); without 'sphere_image' / 'cnn_prediction' that panel is None (:45-51); without an
                EM result the panels are unmarked
      images    one uint8 image per datum, grey or RGB, of the size the lines were detected at
      true_vps  None or per datum None / (K, 3): marked cyan after the result's VPs (:80-83)
      horizons  None or per datum None / two end points in the lines' normalised coordinates"""
    images = list(images)
    hz_px = None
    if horizons is not None:
        hz_px = []
        for im, hz in zip(images, horizons):
            if hz is None:
                hz_px.append(None)
                continue
            h, w = np.asarray(im).shape[:2]
            p = segments_to_pixels([[hz[0][0], hz[0][1], hz[1][0], hz[1][1]]], w, h)[0]
            hz_px.append(((p[0], p[1]), (p[2], p[3])))
    return _render(datums, images, maxbest, true_vps, hz_px, device, cell)


def render_em_result(datum, image, maxbest=4, true_vps=None, horizon=None, device=0, cell=10):
    """render_em_results_batch for one datum: the dict of its three panels."""
    return render_em_results_batch([datum], [image], maxbest, [true_vps], [horizon], device, cell)[0]


def plot_result(panel, vps, angles, vp_counts, best=None, img_size=250, std_mark='yo', device=0):
    """plot_result's 2-D branch (:113-139) on one square panel: returns the panel as uint8 RGB with one disc per VP.
    ``panel`` is img_size * c pixels wide for a whole c >= 1 (c = 1: the sphere image; c = 10: response_panel's output);
    ``std_mark`` is one of the reference's 'yo', 'go', 'co'.  Without ``vp_counts`` every disc has diameter 6."""
    rgb = to_rgb(panel)
    side = rgb.shape[0]
    if rgb.shape[1] != side or side % int(img_size) != 0:
        raise ValueError("the panel must be square and a whole multiple of img_size = %d wide (got %s)" % (img_size, rgb.shape[:2]))
    c = side // int(img_size)
    marks = marker_primitives(vps, angles, vp_counts, best, img_size=int(img_size), std_mark=std_mark, cell=c)
    return overlay_batch([rgb], [marks], True, device)[0]


def show_em_result(datum, image_file, maxbest=4, true_vps=None, target_size=None, horizon=None, out_file=None, device=0):
    """show_em_result (:11-110) without a display: reads ``image_file`` (frontend.imread), scales it to fit
    ``target_size`` when given (frontend.resize_to_fit, :15-20), renders and returns the dict of the three panels.
    ``horizon``: two end points in PIXEL coordinates of the (resized) image, as the reference's caller passes them
    (example.py:65-82).  ``out_file``: the image panel is written there (PIL picks the format from the suffix)."""
    from . import frontend
    image = frontend.imread(image_file)
    if target_size is not None:
        image = frontend.resize_to_fit(image, target_size)
    panels = _render([datum], [image], maxbest, [true_vps], [horizon], device, 10)[0]
    if out_file is not None:
        from PIL import Image
        Image.fromarray(panels['image']).save(out_file)
    return panels
