"""The call surface of the reference's probability_functions.py (same names, same signatures), evaluated on the GPU:
pdf_params (:62-96) by vpk_prior_params, calc_pdf (:8-40) by vpk_mixture_pdf, and the E-step -- calc_probabilities
(:99-120) with the calc_lvsq_* family (:150-249) -- by vpk_estep_batch (include/vpk.h), for all three distance measures.

The reference's names take and return NumPy arrays.  The ``*_batch`` forms beside them take many images at once and
return device tensors.  There is no host fallback: without the library and a GPU every density, distance and probability
call raises.  Three functions are host NumPy by design and need no GPU: calc_angles, calc_plv (:133-147) and calc_pvl
(:123-130).  The last two take a caller's lvsq / p_lv matrix, which no kernel reads: they are the reference's own few
NumPy lines (bit-equal to it), for callers that hold such a matrix already.  They are not a fallback for anything:
inside calc_probabilities both stages run in the kernel, and nothing else in this module computes on the host.

Deliberate differences of the E-step from the reference:
  - the caller's ``s`` is not written (calc_plv floors it in place at :139); calc_probabilities_batch returns the floored
    values;
  - an unknown ``distance_measure`` raises ValueError (the reference falls through to a NameError at :114);
  - p_l is one sum over the VPs in ascending order, not np.dot's BLAS order (:116).
The "area" measure is kept as the reference has it: np.cross of the 2-vector v_ (:200) measures from the line through the
segment's midpoint in direction v_.  vp_localisation's calc_vp_line_counts_batch and merge_vps_batch take the three
measures too; the EM runs "angle" and "dotprod" (the reference asserts on "area" there), split_best_vp has no measure.

Not here: calc_point (:261-266; dead, it overwrites its own first column) and calc_vp_line_triangles (no caller)."""
from collections import namedtuple

import numpy as np

from . import ragged
from .ragged import offsets_of as _offsets_of    # the name tests/test_gpu_estep_surface.py builds its offsets with
from ._lib import VPK_DIST
from .runtime import get_runtime

PDFParams = namedtuple('PDFParams', 'means weights sigma')
PDF = namedtuple('PDF', 'v lv vl l lvsq angles')

GRID = 20     # the CNN's response map is GRID x GRID (cnn/deploy.prototxt:283-296)


def _sigma(confidence):
    # confidence = 1.645: 90 %, 1.282: 80 %, 1.000: 68 % (:67-69)
    sigma = np.pi / (confidence * GRID)                         # :71
    if not sigma > 0:
        raise ValueError("confidence must be positive")
    return sigma


def _grid_means():
    """means of pdf_params (:73-80, :92-94): alpha varies along a row of the map, beta along a column."""
    A = B = GRID
    alphas = np.tile(np.linspace(-(A - 1.0) / A * np.pi / 2, (A - 1.0) / A * np.pi / 2, A), (B, 1))
    betas = np.tile(np.linspace(-(B - 1.0) / B * np.pi / 2, (B - 1.0) / B * np.pi / 2, B), (A, 1)).T
    means = np.zeros((A * B, 2))
    means[:, 0] = alphas.flatten()
    means[:, 1] = betas.flatten()
    return means


def _check_maps(maps):
    """Batch size of (B, 20, 20) response maps (one map: (20, 20)); anything else raises before the GPU is touched."""
    shape = tuple(maps.shape)
    if shape == (GRID, GRID):
        return 1
    if len(shape) != 3 or shape[1:] != (GRID, GRID):
        raise ValueError("response maps must be %d x %d (got %r)" % (GRID, GRID, shape))
    return shape[0]


def _is_params(x):
    return hasattr(x, 'means') and hasattr(x, 'weights')


def _maps_to_device(rt, maps):
    """The response maps as a (B, 400) float32 device tensor.  The kernels only read it, so the caller's maps are never
    written, also where no copy is made."""
    return ragged.to_device(rt, maps, np.float32).reshape(_check_maps(maps), GRID * GRID)


def _prior_weights(rt, d_maps, sigma):
    w = rt.torch.empty_like(d_maps)
    rt.check(rt.lib.vpk_prior_params(rt.h, int(d_maps.shape[0]), rt.ptr(d_maps), float(sigma), rt.ptr(w)))
    return w


def _mixture(rt, means, weights, sigma, pts, want_angles=False):
    """vpk_mixture_pdf.  means (ncomp, 2) or (B, ncomp, 2); weights (B, ncomp); pts (P, dim) or (B, P, dim), dim 2 or 3;
    all float64 device tensors.  Returns (angles (B, P, 2) or None, pdf (B, P))."""
    t = rt.torch
    batch, ncomp = int(weights.shape[0]), int(weights.shape[1])
    shared_m, shared_p = means.dim() == 2, pts.dim() == 2
    if tuple(means.shape[-2:]) != (ncomp, 2) or (not shared_m and means.shape[0] != batch):
        raise ValueError("means must be (ncomp, 2) or (batch, ncomp, 2) for weights (batch, ncomp)")
    if pts.shape[-1] not in (2, 3) or (not shared_p and pts.shape[0] != batch):
        raise ValueError("points must be (npts, 2 or 3) or (batch, npts, 2 or 3)")
    npts, dim = int(pts.shape[-2]), int(pts.shape[-1])
    pdf = t.empty((batch, npts), dtype=t.float64, device=rt.tdev)
    angles = t.empty((batch, npts, 2), dtype=t.float64, device=rt.tdev) if want_angles else None
    rt.check(rt.lib.vpk_mixture_pdf(rt.h, batch, ncomp, rt.ptr(means), int(shared_m), rt.ptr(weights), float(sigma), npts,
                                    rt.ptr(pts), dim, int(shared_p), rt.ptr(angles), rt.ptr(pdf)))
    return angles, pdf


# ---- batch forms: device tensors --------------------------------------------------------------------------------------
def pdf_params_batch(maps, confidence=1.282, device=0):
    """pdf_params for B response maps at once (B x 20 x 20, NumPy or torch; cast to float32 where they are not).
    Returns PDFParams(means (400, 2) float64 -- one set, every map has the same --, weights (B, 400) float32,
    sigma float), the arrays on the device."""
    _check_maps(maps)
    sigma = _sigma(confidence)
    rt = get_runtime(device)
    with rt.on_stream():
        weights = _prior_weights(rt, _maps_to_device(rt, maps), sigma)
        means = ragged.to_device(rt, _grid_means(), np.float64)
    rt.synchronize()
    return PDFParams(means=means, weights=weights, sigma=sigma)


def _params_on_device(rt, maps_or_params):
    """(means, float64 weights (B, ncomp), sigma) on the device from response maps or from a PDFParams whose weights are
    (ncomp,) or (B, ncomp) and whose means are (ncomp, 2) or (B, ncomp, 2)."""
    t = rt.torch
    if _is_params(maps_or_params):
        means = ragged.to_device(rt, maps_or_params.means, np.float64)
        weights = ragged.to_device(rt, maps_or_params.weights, np.float64)      # a float32 weight enters :38 as its double
        if weights.dim() == 1:
            weights = weights.reshape(1, -1)
        return means, weights, float(maps_or_params.sigma)
    sigma = _sigma(1.282)
    weights = _prior_weights(rt, _maps_to_device(rt, maps_or_params), sigma).double()
    return ragged.to_device(rt, _grid_means(), np.float64), weights, sigma


def calc_pdf_batch(maps_or_params, x, y, device=0):
    """calc_pdf for B mixtures: the density of each at (x[i], y[i]).  ``maps_or_params``: B x 20 x 20 response maps
    (pdf_params' defaults apply) or a PDFParams (pdf_params_batch's, or any means / weights / sigma).  x, y: (P,) -- the
    same points for every mixture -- or (B, P).  Returns a (B, P) float64 device tensor."""
    if not _is_params(maps_or_params):
        _check_maps(maps_or_params)
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        means, weights, sigma = _params_on_device(rt, maps_or_params)
        pts = t.stack((ragged.to_device(rt, x, np.float64), ragged.to_device(rt, y, np.float64)), dim=-1).contiguous()
        _, pdf = _mixture(rt, means, weights, sigma, pts)
    rt.synchronize()
    return pdf


def vp_prior_batch(maps, vps, device=0):
    """PDF.angles and PDF.v of calc_probabilities (:104-105) for candidate VPs: ``vps`` (M, 3) -- the same for every map --
    or (B, M, 3) unit vectors; ``maps`` as in calc_pdf_batch.  Returns (angles (B, M, 2), p_v (B, M)), float64 device
    tensors."""
    if not _is_params(maps):
        _check_maps(maps)
    rt = get_runtime(device)
    with rt.on_stream():
        means, weights, sigma = _params_on_device(rt, maps)
        v = ragged.to_device(rt, vps, np.float64)
        if v.shape[-1] != 3:
            raise ValueError("vps must be (M, 3) or (B, M, 3)")
        angles, pdf = _mixture(rt, means, weights, sigma, v, want_angles=True)
    rt.synchronize()
    return angles, pdf


# ---- the E-step: device tensors -------------------------------------------------------------------------------------------
DISTANCE_MEASURES = dict(VPK_DIST)


def _measure(distance_measure):
    if not isinstance(distance_measure, str) or distance_measure not in DISTANCE_MEASURES:
        raise ValueError("distance_measure %r: one of \"angle\", \"dotprod\", \"area\"" % (distance_measure,))
    return DISTANCE_MEASURES[distance_measure]


def _estep(rt, lo, vo, d_lp, d_l, d_v, d_s, d_pv, measure, want):
    """vpk_estep_batch: the outputs named in ``want`` ('s', 'lvsq', 'p_lv', 'p_l', 'p_vl') as flat device tensors."""
    t = rt.torch
    total = int((np.diff(lo) * np.diff(vo)).sum())
    shapes = {'s': int(vo[-1]), 'lvsq': total, 'p_lv': total, 'p_l': int(lo[-1]), 'p_vl': total}
    # the matrices are written in full wherever an image has lines and VPs, and have no elements elsewhere; s and p_l of an
    # image that gets no workgroup stay 0
    out = {k: ((t.zeros if k in ('s', 'p_l') else t.empty)((shapes[k],), dtype=t.float64, device=rt.tdev) if k in want else None)
           for k in shapes}
    rt.check(rt.lib.vpk_estep_batch(rt.h, lo.shape[0] - 1, ragged.off_ptr(lo), ragged.off_ptr(vo), rt.ptr(d_lp), rt.ptr(d_l),
                                    rt.ptr(d_v), rt.ptr(d_s), rt.ptr(d_pv), measure, rt.ptr(out['s']), rt.ptr(out['lvsq']),
                                    rt.ptr(out['p_lv']), rt.ptr(out['p_l']), rt.ptr(out['p_vl'])))
    return out


def _estep_offsets(vs, ls, lps, measure):
    """(line offsets, VP offsets) of the E-step's lists, every image held to its row shape; host only."""
    lo = ragged.strict_offsets(lps, (4,), "lps")
    vo = ragged.strict_offsets(vs, (3,), "vs")
    if lo.shape != vo.shape:
        raise ValueError("lps and vs describe %d and %d images" % (lo.shape[0] - 1, vo.shape[0] - 1))
    if measure == DISTANCE_MEASURES["dotprod"]:
        if ls is None or any(x is None for x in ls):
            raise ValueError("the \"dotprod\" measure reads the homogeneous lines: ls is needed")
        if not np.array_equal(ragged.strict_offsets(ls, (3,), "ls"), lo):
            raise ValueError("ls and lps differ in their images' line counts")
    return lo, vo


def _estep_inputs(rt, vs, ls, lps, measure):
    d_lp, d_v = ragged.upload(rt, lps, np.float64, (4,)), ragged.upload(rt, vs, np.float64, (3,))
    return d_lp, ragged.upload(rt, ls, np.float64, (3,)) if measure == DISTANCE_MEASURES["dotprod"] else None, d_v


def calc_lvsq_batch(vs, ls, lps, distance_measure="angle", device=0):
    """calc_lvsq_angle / _dotprod / _area for many images in one launch.  ``vs``: per image the VPs (M_b, 3); ``ls``: per
    image the homogeneous lines (N_b, 3) -- read by "dotprod" only, else it may be None --; ``lps``: per image the end
    points (N_b, 4); NumPy arrays or tensors.  Returns a list with one (N_b, M_b) float64 device tensor per image: the
    transposed view of the kernel's [m][n] buffer.  Any M_b; an image without lines or VPs gives an empty matrix.  No
    chain crosses the VPs here, so the launch also splits the VP range: a few lines against thousands of hypotheses still
    fill the machine."""
    measure = _measure(distance_measure)
    lo, vo = _estep_offsets(vs, ls, lps, measure)
    rt = get_runtime(device)
    with rt.on_stream():
        d_lp, d_l, d_v = _estep_inputs(rt, vs, ls, lps, measure)
        d_s = rt.torch.ones((int(vo[-1]),), dtype=rt.torch.float64, device=rt.tdev)
        out = _estep(rt, lo, vo, d_lp, d_l, d_v, d_s, None, measure, ('lvsq',))
    rt.synchronize()
    return ragged.split_mats(out['lvsq'], lo, vo, True)


def _prior_ragged(rt, pdfpars_or_maps, d_v, vo):
    """(angles (sum M, 2), p_v (sum M,)) of a ragged batch of VP sets through ONE vpk_mixture_pdf launch: the sets are padded
    to the largest with the image centre, and the padding is dropped again by an index made from the host offsets."""
    t = rt.torch
    B = vo.shape[0] - 1
    means, weights, sigma = _params_on_device(rt, pdfpars_or_maps)
    if weights.shape[0] == 1 and B > 1 and means.dim() == 2:
        weights = weights.expand(B, -1).contiguous()
    if weights.shape[0] != B:
        raise ValueError("%d priors for %d images" % (weights.shape[0], B))
    sizes = np.diff(vo)
    mmax = int(sizes.max()) if B else 0
    if B == 0 or mmax == 0:
        return (t.zeros((0, 2), dtype=t.float64, device=rt.tdev), t.zeros((0,), dtype=t.float64, device=rt.tdev))
    idx = np.concatenate([b * mmax + np.arange(int(sizes[b]), dtype=np.int64) for b in range(B)])
    d_idx = t.from_numpy(idx).to(rt.tdev)
    pad = t.zeros((B * mmax, 3), dtype=t.float64, device=rt.tdev)
    pad[:, 2] = 1.0
    pad[d_idx] = d_v
    angles, pdf = _mixture(rt, means, weights, sigma, pad.reshape(B, mmax, 3), want_angles=True)
    return angles.reshape(B * mmax, 2)[d_idx].contiguous(), pdf.reshape(B * mmax)[d_idx].contiguous()


def calc_probabilities_batch(pdfpars_or_maps, vs, ls, lps, ss, distance_measure="angle", device=0):
    """calc_probabilities for many images: the prior of every VP (one vpk_mixture_pdf launch) and the E-step (one
    vpk_estep_batch launch).  ``pdfpars_or_maps``: B x 20 x 20 response maps (pdf_params' defaults apply) or a PDFParams
    (pdf_params_batch's, or any means / weights (B, ncomp) / sigma; one weight row serves every image); ``vs``, ``ls``,
    ``lps`` as in calc_lvsq_batch; ``ss``: per image the variances (M_b,).  Nothing is copied to the host.  Returns a dict:
    'pdf' a list with one PDF tuple per image -- v (M,), lv (N, M), vl (M, N), l (N,), lvsq (N, M), angles (M, 2), float64
    device tensors, lv and lvsq transposed views of [m][n] buffers --, 's' a list of the variances floored at 1e-200 (the
    caller's are not written), and the host offsets 'line_offsets' and 'vp_offsets'."""
    measure = _measure(distance_measure)
    if not _is_params(pdfpars_or_maps):
        _check_maps(pdfpars_or_maps)
    lo, vo = _estep_offsets(vs, ls, lps, measure)
    if not np.array_equal(ragged.strict_offsets(ss, (), "ss"), vo):
        raise ValueError("ss and vs differ in their images' VP counts")
    rt = get_runtime(device)
    with rt.on_stream():
        d_lp, d_l, d_v = _estep_inputs(rt, vs, ls, lps, measure)
        d_s = ragged.upload(rt, ss, np.float64)
        angles, p_v = _prior_ragged(rt, pdfpars_or_maps, d_v, vo)
        out = _estep(rt, lo, vo, d_lp, d_l, d_v, d_s, p_v, measure, ('s', 'lvsq', 'p_lv', 'p_l', 'p_vl'))
    rt.synchronize()
    lvsq, p_lv, p_vl = (ragged.split_mats(out[k], lo, vo, k != 'p_vl') for k in ('lvsq', 'p_lv', 'p_vl'))
    pdfs, s_out = [], []
    for b in range(lo.shape[0] - 1):
        n0, n1, m0, m1 = int(lo[b]), int(lo[b + 1]), int(vo[b]), int(vo[b + 1])
        pdfs.append(PDF(v=p_v[m0:m1], lv=p_lv[b], vl=p_vl[b], l=out['p_l'][n0:n1], lvsq=lvsq[b], angles=angles[m0:m1]))
        s_out.append(out['s'][m0:m1])
    return {'pdf': pdfs, 's': s_out, 'line_offsets': lo, 'vp_offsets': vo}


def _grid_xy(N):
    X = np.arange(-np.pi / 2, np.pi / 2, np.pi * 1.0 / N)       # :277-279
    Y = np.arange(-np.pi / 2, np.pi / 2, np.pi * 1.0 / N)
    return np.meshgrid(X, Y)


def pdf_grid_batch(maps, N=50, device=0):
    """pdf_grid for B response maps: {'X', 'Y'} the reference's N x N mesh (NumPy, shared), 'p' a (B, N, N) float64
    device tensor with p[b, i, j] the density of map b at (X[i, j], Y[i, j])."""
    X, Y = _grid_xy(N)
    p = calc_pdf_batch(maps, X.ravel(), Y.ravel(), device=device)
    return {'X': X, 'Y': Y, 'p': p.reshape((p.shape[0],) + X.shape)}


# ---- the reference's names: NumPy in, NumPy out ------------------------------------------------------------------------
def pdf_params(cnn_response, confidence=1.282, device=0):
    """pdf_params (:62-96): PDFParams(means (400, 2) float64, weights (400,) float32, sigma).  The weights come from the
    device (the rule the EM's prior uses); the caller's map is left untouched, as in the reference, whose flatten() copies.
    A map that is not float32 is cast to float32 first -- the reference would carry the map's own precision through the
    normalisation.  Maps other than 20 x 20 raise ValueError."""
    if tuple(np.shape(cnn_response)) != (GRID, GRID):
        raise ValueError("cnn_response must be %d x %d (got %r)" % (GRID, GRID, tuple(np.shape(cnn_response))))
    par = pdf_params_batch(np.asarray(cnn_response)[None], confidence=confidence, device=device)
    return PDFParams(means=_grid_means(), weights=par.weights[0].cpu().numpy(), sigma=par.sigma)


def calc_angles(M, v):
    angle = np.zeros((M, 2))
    angle[:, 1] = np.arcsin(v[:, 1])
    inner = v[:, 0] / np.cos(angle[:, 1])
    inner = np.minimum(inner, 1)
    inner = np.maximum(inner, -1)
    angle[:, 0] = np.arcsin(inner)
    return angle


def calc_pdf(pdfpar, x, y, device=0):
    """calc_pdf (:8-40) for any PDFParams (any means, component count and sigma): the density at (x[i], y[i])."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    par = PDFParams(means=np.asarray(pdfpar.means), weights=np.asarray(pdfpar.weights).reshape(1, -1), sigma=pdfpar.sigma)
    return calc_pdf_batch(par, x, y, device=device)[0].cpu().numpy()


def calc_pdf_grid(pdfpar, X, Y, device=0):
    """What calc_pdf_grid (:43-59) intends: response[:, j] = calc_pdf(pdfpar, X[:, j], Y[:, j]) for every column.  (The
    reference itself raises TypeError at :54, np.zeros((X.shape,)), and so never returns.)"""
    means = np.asarray(pdfpar.means)
    weights = np.asarray(pdfpar.weights)
    if not weights.shape[0] == means.shape[0]:                  # :50-52
        print("means has wrong shape!")
        return 0
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    return calc_pdf(pdfpar, X.ravel(), Y.ravel(), device=device).reshape(X.shape)


def pdf_grid(cnn_response, N=50, device=0):
    """pdf_grid (:269-296): {'X', 'Y', 'p'} -- the prior density of one response map on an N x N mesh."""
    pdfpar = pdf_params(cnn_response, device=device)
    X, Y = _grid_xy(N)
    return {'X': X, 'Y': Y, 'p': calc_pdf_grid(pdfpar, X, Y, device=device)}


# ---- the E-step: the reference's names --------------------------------------------------------------------------------
def calc_probabilities(i, pdfpar, v, l, lp, s, llen, distance_measure="angle", device=0):
    """calc_probabilities (:99-120) on slice i of the history array ``v`` (iterations, M, 3): the PDF tuple v (M,), lv (N, M),
    vl (M, N), l (N,), lvsq (N, M), angles (M, 2) that EM_result['distribution'] uses.  ``llen`` is read by no measure.
    ``s`` is not written (see the module's list of differences)."""
    _measure(distance_measure)
    vi = np.asarray(v, dtype=np.float64)[i].reshape(-1, 3)
    par = PDFParams(means=np.asarray(pdfpar.means), weights=np.asarray(pdfpar.weights).reshape(1, -1), sigma=pdfpar.sigma)
    r = calc_probabilities_batch(par, [vi], [None if l is None else np.asarray(l, dtype=np.float64).reshape(-1, 3)],
                                 [np.asarray(lp, dtype=np.float64).reshape(-1, 4)],
                                 [np.asarray(s, dtype=np.float64).reshape(-1)], distance_measure=distance_measure,
                                 device=device)['pdf'][0]
    return PDF(*(np.ascontiguousarray(x.cpu().numpy()) for x in r))


def calc_pvl(M, N, p_lv, p_v, p_l):
    """calc_pvl (:123-130) on a caller's matrices, in NumPy (see the module docstring): p_vl[m, n] = p_lv[n, m] p_v[m] / p_l[n]."""
    p_lv, p_v, p_l = np.asarray(p_lv), np.asarray(p_v), np.asarray(p_l)
    return (p_lv[:N, :M] * p_v[None, :M]).T / p_l[None, :N]


def calc_plv(M, v, s, lvsq, lp):
    """calc_plv (:133-147) on a caller's lvsq (N, M), in NumPy (see the module docstring).  The caller's s is not written."""
    s = np.asarray(s, dtype=np.float64)[:M]
    sf = np.where(s > 1e-200, s, 1e-200)                        # :139
    p_lv = np.exp(-(np.asarray(lvsq, dtype=np.float64) / (2 * sf)[None, :]))
    return p_lv * (1.0 / np.sqrt(2 * np.pi * sf))[None, :]


def _calc_lvsq(v, l, lp, distance_measure, device):
    v = np.asarray(v, dtype=np.float64).reshape(3, -1)
    ls = None if l is None else [np.asarray(l, dtype=np.float64).reshape(-1, 3)]
    out = calc_lvsq_batch([np.ascontiguousarray(v.T)], ls, [np.asarray(lp, dtype=np.float64).reshape(-1, 4)],
                          distance_measure=distance_measure, device=device)[0]
    return np.ascontiguousarray(out.cpu().numpy())


def calc_lvsq_dotprod(v, l, lp, llen, device=0):
    """calc_lvsq_dotprod (:150-154): ``v`` 3 x M as in the reference, ``l`` (N, 3); returns (N, M)."""
    return _calc_lvsq(v, l, lp, "dotprod", device)


def calc_lvsq_angle(v, l, lp, llen, device=0):
    """calc_lvsq_angle (:157-176): ``v`` 3 x M, ``lp`` (N, 4); returns (N, M).  ``l`` and ``llen`` are not read."""
    return _calc_lvsq(v, None, lp, "angle", device)


def calc_lvsq_area(v, l, lp, llen, device=0):
    """calc_lvsq_area (:179-209): ``v`` 3 x M, ``lp`` (N, 4); returns (N, M).  ``l`` and ``llen`` are not read."""
    return _calc_lvsq(v, None, lp, "area", device)


def calc_lvsq_single(v, l, lp, device=0):
    """calc_lvsq_single (:212-224): one VP (3,) against one segment (4,)."""
    return _calc_lvsq(np.asarray(v, dtype=np.float64).reshape(3, 1), None, np.asarray(lp, dtype=np.float64).reshape(1, 4),
                      "angle", device)[0, 0]


def calc_lvsq_area_single(v, l, lp, device=0):
    """calc_lvsq_area_single (:227-249): one VP (3,) against one segment (4,)."""
    return _calc_lvsq(np.asarray(v, dtype=np.float64).reshape(3, 1), None, np.asarray(lp, dtype=np.float64).reshape(1, 4),
                      "area", device)[0, 0]


def vp_is_within_image(vp):
    vp2 = vp[0:2] / vp[2]
    if vp2[0] < 2 and vp2[0] > -2 and vp2[1] < 2 and vp2[1] > -2:
        return True
    else:
        return False
