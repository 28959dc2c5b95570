"""The prior's call surface of the reference's probability_functions.py (same names, same signatures), evaluated on
the GPU: pdf_params (:62-96) by vpk_prior_params, calc_pdf (:8-40) by vpk_mixture_pdf (include/vpk.h).

The reference's names take and return NumPy arrays.  The ``*_batch`` forms beside them take many response maps at once
and return device tensors.  There is no host fallback: without the library and a GPU every density call raises.

Not here: calc_probabilities, calc_plv, calc_pvl and the calc_lvsq_* family (the E-step lives in the EM workgroup;
vpk_estep is its fine-grained entry)."""
from collections import namedtuple

import numpy as np

PDFParams = namedtuple('PDFParams', 'means weights sigma')
PDF = namedtuple('PDF', 'v lv vl l lvsq angles')

GRID = 20     # the CNN's response map is GRID x GRID (cnn/deploy.prototxt:283-296)


def _runtime(device):
    from .runtime import get_runtime
    return get_runtime(device)


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


def _to_device(rt, a, dtype):
    """``a`` (NumPy array or torch tensor, any device) as a contiguous tensor of ``dtype`` on the runtime's GPU."""
    t = rt.torch
    if not isinstance(a, t.Tensor):
        a = t.from_numpy(np.ascontiguousarray(a))
    return a.to(device=rt.tdev, dtype=dtype).contiguous()


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
    return _to_device(rt, maps, rt.torch.float32).reshape(_check_maps(maps), GRID * GRID)


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
    rt = _runtime(device)
    with rt.on_stream():
        weights = _prior_weights(rt, _maps_to_device(rt, maps), sigma)
        means = _to_device(rt, _grid_means(), rt.torch.float64)
    rt.synchronize()
    return PDFParams(means=means, weights=weights, sigma=sigma)


def _params_on_device(rt, maps_or_params):
    """(means, float64 weights (B, ncomp), sigma) on the device from response maps or from a PDFParams whose weights are
    (ncomp,) or (B, ncomp) and whose means are (ncomp, 2) or (B, ncomp, 2)."""
    t = rt.torch
    if _is_params(maps_or_params):
        means = _to_device(rt, maps_or_params.means, t.float64)
        weights = _to_device(rt, maps_or_params.weights, t.float64)      # a float32 weight enters :38 as its double
        if weights.dim() == 1:
            weights = weights.reshape(1, -1)
        return means, weights, float(maps_or_params.sigma)
    sigma = _sigma(1.282)
    weights = _prior_weights(rt, _maps_to_device(rt, maps_or_params), sigma).double()
    return _to_device(rt, _grid_means(), t.float64), weights, sigma


def calc_pdf_batch(maps_or_params, x, y, device=0):
    """calc_pdf for B mixtures: the density of each at (x[i], y[i]).  ``maps_or_params``: B x 20 x 20 response maps
    (pdf_params' defaults apply) or a PDFParams (pdf_params_batch's, or any means / weights / sigma).  x, y: (P,) -- the
    same points for every mixture -- or (B, P).  Returns a (B, P) float64 device tensor."""
    if not _is_params(maps_or_params):
        _check_maps(maps_or_params)
    rt = _runtime(device)
    t = rt.torch
    with rt.on_stream():
        means, weights, sigma = _params_on_device(rt, maps_or_params)
        pts = t.stack((_to_device(rt, x, t.float64), _to_device(rt, y, t.float64)), dim=-1).contiguous()
        _, pdf = _mixture(rt, means, weights, sigma, pts)
    rt.synchronize()
    return pdf


def vp_prior_batch(maps, vps, device=0):
    """PDF.angles and PDF.v of calc_probabilities (:104-105) for candidate VPs: ``vps`` (M, 3) -- the same for every map --
    or (B, M, 3) unit vectors; ``maps`` as in calc_pdf_batch.  Returns (angles (B, M, 2), p_v (B, M)), float64 device
    tensors."""
    if not _is_params(maps):
        _check_maps(maps)
    rt = _runtime(device)
    with rt.on_stream():
        means, weights, sigma = _params_on_device(rt, maps)
        v = _to_device(rt, vps, rt.torch.float64)
        if v.shape[-1] != 3:
            raise ValueError("vps must be (M, 3) or (B, M, 3)")
        angles, pdf = _mixture(rt, means, weights, sigma, v, want_angles=True)
    rt.synchronize()
    return angles, pdf


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


def vp_is_within_image(vp):
    vp2 = vp[0:2] / vp[2]
    if vp2[0] < 2 and vp2[0] > -2 and vp2[1] < 2 and vp2[1] > -2:
        return True
    else:
        return False
