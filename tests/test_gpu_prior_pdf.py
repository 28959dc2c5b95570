"""vpk_prior_params and vpk_mixture_pdf (csrc/vpk_prior.hip) and the probability_functions call surface on top of them,
against the reference's stored output (tests/golden/prior/prior_pdf.npz; the bar: tests/prior_reference.py).

Shapes: a workgroup covers 64 points of one image and stages 128 components at a time, so npts = 1, 63, 64, 65 and 300
(one lane, a tile short of / equal to / one past a wave, five tiles), ncomp = 400 (four chunks, the last of 16) with 100, 7
and 0 live components, ncomp = 130 (one component past a chunk), batch 1, 3 and 6, points shared and per image."""
import ctypes
import functools

import numpy as np
import pytest

import prior_reference as R
from golden_util import load

pytestmark = pytest.mark.gpu

VPK_ERR_ARG = -1
NPTS = [1, 63, 64, 65, 300]


@functools.lru_cache(maxsize=None)
def G():
    return R.golden()


def _rt():
    from vanishing_points_2017_amd.runtime import get_runtime
    return get_runtime(0)


def _dev(a, dtype=np.float64):
    rt = _rt()
    return rt.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(rt.tdev)


def mixture(means, weights, sigma, pts, want_angles=False):
    """vpk_mixture_pdf on host arrays: means (ncomp, 2) or (B, ncomp, 2), weights (B, ncomp), pts (P, d) or (B, P, d)."""
    from vanishing_points_2017_amd import probability_functions as prob
    rt = _rt()
    with rt.on_stream():
        ang, pdf = prob._mixture(rt, _dev(means), _dev(weights), sigma, _dev(pts), want_angles=want_angles)
    rt.synchronize()
    return (None if ang is None else ang.cpu().numpy()), pdf.cpu().numpy()


def rolled(a, batch_maps, axis=0):
    """Per-image inputs from a shared list: image k gets the list rotated by 37 k."""
    return np.stack([np.roll(a, 37 * k, axis=axis) for k in range(len(batch_maps))])


@pytest.mark.parametrize("npts", NPTS)
def test_mixture_pdf_every_map_at_the_tile_edges(npts):
    """Every stored map (100, 100, 100, 7, 100 and 0 live components of 400) at the last npts stored points: all six in one
    call, each alone (batch 1), and three different ones with shared points and with points per image."""
    g = G()
    assert [(w > 0).sum() for w in g["weights"]] == [100, 100, 100, 7, 100, 0]
    pts, ref = g["pts"][-npts:], g["pdf"][:, -npts:]          # the tail: the corners, the means, the underflows, the NaN
    _, pdf = mixture(g["means"], g["weights"], g["sigma"], pts)
    print("npts=%d batch 6: worst error / bar %.3g" % (npts, R.check_pdf(pdf, ref, "batch 6")))
    for b in range(6):
        _, one = mixture(g["means"], g["weights"][b:b + 1], g["sigma"], pts)
        R.check_pdf(one, ref[b:b + 1], "map %d alone" % b)
        assert np.array_equal(one[0], pdf[b], equal_nan=True), "map %d: other bits alone than in the batch" % b
    sel = [3, 0, 5]
    _, three = mixture(g["means"], g["weights"][sel], g["sigma"], pts)
    R.check_pdf(three, ref[sel], "batch 3, shared points")
    _, per = mixture(g["means"], g["weights"][sel], g["sigma"], rolled(pts, sel))
    R.check_pdf(per, np.stack([np.roll(ref[b], 37 * k) for k, b in enumerate(sel)]), "batch 3, points per image")


def test_arbitrary_mixture_through_calc_pdf():
    """calc_pdf(pdfpar, x, y) with 130 components of arbitrary means (one past an LDS chunk), weights 0, negative and NaN
    among them, and a sigma of its own; the same mixture with means per image through the C entry."""
    from vanishing_points_2017_amd import probability_functions as prob
    g = G()
    par = prob.PDFParams(means=g["arb_means"], weights=g["arb_weights"], sigma=float(g["arb_sigma"]))
    got = prob.calc_pdf(par, g["pts"][:70, 0], g["pts"][:70, 1])
    print("worst error / bar %.3g" % R.check_pdf(got, g["arb_pdf"], "calc_pdf"))
    order = np.arange(130)[::-1]
    means = np.stack([g["arb_means"], g["arb_means"][order]])
    _, two = mixture(means, np.stack([g["arb_weights"], g["arb_weights"][order]]), float(g["arb_sigma"]), g["pts"][:70])
    R.check_pdf(two[:1], g["arb_pdf"][None], "means per image, image 0")
    assert np.array_equal(two[0], got, equal_nan=True)
    # reversed components add up in another order: sums of non-negative terms, so n u of the sum on top of the bar
    ok = ~np.isnan(g["arb_pdf"])
    assert np.all(np.abs(two[1][ok] - g["arb_pdf"][ok]) <= (130 * 2.0 ** -52 + R.PDF_RTOL) * g["arb_pdf"][ok])


@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per-image"])
def test_vector_form(per_image):
    """pts_dim = 3: the angles within 4 ulp of the reference's (the device's asin and cos against libm's, each within an
    ulp: tests/test_gpu_math.py; asin of an argument that is off by two), the densities at the bar.  (0, +-1, 0) divides
    by cos(+-pi/2), (+-1, 0, 0) lands on the clip."""
    g = G()
    vecs = rolled(g["vecs"], range(6)) if per_image else g["vecs"]
    want_a = rolled(g["angles"], range(6)) if per_image else np.broadcast_to(g["angles"], (6, 64, 2))
    want_p = np.stack([np.roll(g["pdf_vec"][b], 37 * b) for b in range(6)]) if per_image else g["pdf_vec"]
    ang, pdf = mixture(g["means"], g["weights"], g["sigma"], vecs, want_angles=True)
    ulp = R.ulp_distance(ang, want_a)
    print("angles: worst %d ulp; densities: worst error / bar %.3g" % (ulp.max(), R.check_pdf(pdf, want_p, "vectors")))
    assert ulp.max() <= 4
    _, without = mixture(g["means"], g["weights"], g["sigma"], vecs)
    assert np.array_equal(without, pdf, equal_nan=True)


@pytest.mark.parametrize("name", ["yud_n120", "clean3_n60"])
def test_vp_prior_batch_against_the_references_last_estep(name):
    """PDF.v and PDF.angles of the reference's own last calc_probabilities call (tests/golden/dist_<case>.npz) from the
    final VPs and the response map."""
    from vanishing_points_2017_amd import probability_functions as prob
    case, dist = load(name), load("dist_" + name)
    angles, p_v = prob.vp_prior_batch(case["cnn_response"][None], case["o_vp"])
    assert tuple(angles.shape) == (1,) + dist["angles"].shape and tuple(p_v.shape) == (1,) + dist["p_v"].shape
    ulp = R.ulp_distance(angles[0].cpu().numpy(), dist["angles"])
    print("%s: angles worst %d ulp; p_v worst error / bar %.3g" % (
        name, ulp.max(), R.check_pdf(p_v[0].cpu().numpy(), dist["p_v"], name)))
    assert ulp.max() <= 4
    _, again = prob.vp_prior_batch(np.stack([case["cnn_response"]] * 2), np.stack([case["o_vp"]] * 2))
    assert np.array_equal(again[0].cpu().numpy(), p_v[0].cpu().numpy()) and np.array_equal(again[1].cpu().numpy(), p_v[0].cpu().numpy())


def test_prior_params_are_the_references_and_the_ems():
    """All maps in one call: the reference's float32 weights bit for bit (NaN for the all-zero map), and what vpk_init_vps
    reports for each map (the EM's own prior).  pdf_params leaves the caller's map alone, casts float64 maps, honours
    `confidence` (against oracle.em_numpy.pdf_params) and rejects other shapes."""
    from vanishing_points_2017_amd import kernels, probability_functions as prob
    from oracle import em_numpy as em
    g = G()
    par = prob.pdf_params_batch(g["maps"])
    w = par.weights.cpu().numpy()
    assert w.dtype == np.float32 and w.shape == (6, 400)
    assert np.array_equal(w, g["weights"], equal_nan=True)
    assert np.array_equal(par.means.cpu().numpy(), g["means"]) and par.sigma == float(g["sigma"])
    sphere = load("yud_n120")["sphere_image"]
    for b in range(6):
        _, w_em = kernels.init_vps(g["maps"][b], sphere)
        assert np.array_equal(w_em, w[b], equal_nan=True), "map %d: not the EM's prior" % b
    one = g["maps"][1].copy()
    single = prob.pdf_params(one)
    assert np.array_equal(one, g["maps"][1])
    assert single.weights.dtype == np.float32 and np.array_equal(single.weights, g["weights"][1])
    assert np.array_equal(single.means, g["means"]) and single.sigma == float(g["sigma"])
    assert np.array_equal(prob.pdf_params(g["maps"][1].astype(np.float64)).weights, g["weights"][1])
    for conf in (1.0, 1.645):
        want = em.pdf_params(g["maps"][4].copy(), confidence=conf)
        got = prob.pdf_params(g["maps"][4], confidence=conf)
        assert got.sigma == want.sigma and np.array_equal(got.weights, want.weights)
    with pytest.raises(ValueError):
        prob.pdf_params(np.zeros((20, 21), dtype=np.float32))


def test_pdf_grid():
    """pdf_grid(map, N = 8): the reference's X and Y, p column by column what calc_pdf gives (the bar; the oracle's
    calc_pdf as a second opinion), and pdf_grid_batch / calc_pdf_batch the same numbers for several maps."""
    from vanishing_points_2017_amd import probability_functions as prob
    from oracle import em_numpy as em
    g = G()
    out = prob.pdf_grid(g["maps"][0], N=8)
    X, Y = np.meshgrid(np.arange(-np.pi / 2, np.pi / 2, np.pi / 8), np.arange(-np.pi / 2, np.pi / 2, np.pi / 8))
    assert np.array_equal(out["X"], X) and np.array_equal(out["Y"], Y) and out["p"].shape == (8, 8)
    par = prob.pdf_params(g["maps"][0])
    ref_par = em.PDFParams(means=g["means"], weights=g["weights"][0], sigma=float(g["sigma"]))
    for j in range(8):
        R.check_pdf(out["p"][:, j], prob.calc_pdf(par, X[:, j], Y[:, j]), "column %d" % j)
        R.check_pdf(out["p"][:, j], em.calc_pdf(ref_par, X[:, j], Y[:, j]), "column %d against the oracle" % j)
    assert np.array_equal(prob.calc_pdf_grid(par, X, Y), out["p"])
    many = prob.pdf_grid_batch(g["maps"], N=8)
    p = many["p"].cpu().numpy()
    assert p.shape == (6, 8, 8) and np.array_equal(many["X"], X) and np.array_equal(p[0], out["p"])
    assert not p[5].any() and not np.isnan(p).any()
    flat = prob.calc_pdf_batch(prob.pdf_params_batch(g["maps"]), X.ravel(), Y.ravel()).cpu().numpy()
    assert np.array_equal(flat.reshape(6, 8, 8), p)


def test_bad_arguments_and_empty_calls():
    rt = _rt()
    g = G()
    t = rt.torch
    with rt.on_stream():
        means, w, pts = _dev(g["means"]), _dev(g["weights"][:2]), _dev(g["pts"][:10])
        maps = _dev(g["maps"][:2].reshape(2, 400), np.float32)
        out = t.full((2, 10), -7.0, dtype=t.float64, device=rt.tdev)
        wout = t.full((2, 400), -7.0, dtype=t.float32, device=rt.tdev)
    rt.synchronize()
    P = rt.ptr

    def pdf(batch=2, ncomp=400, sigma=0.1, npts=10, dim=2, m=means, ww=w, p=pts, o=out):
        return rt.lib.vpk_mixture_pdf(rt.h, batch, ncomp, P(m), 1, P(ww), ctypes.c_double(sigma), npts, P(p), dim, 1, None, P(o))

    assert pdf(batch=-1) == VPK_ERR_ARG and pdf(ncomp=-1) == VPK_ERR_ARG and pdf(npts=-1) == VPK_ERR_ARG
    assert pdf(sigma=0.0) == VPK_ERR_ARG and pdf(sigma=-1.0) == VPK_ERR_ARG and pdf(sigma=float("nan")) == VPK_ERR_ARG
    assert pdf(dim=1) == VPK_ERR_ARG and pdf(dim=4) == VPK_ERR_ARG
    assert pdf(m=None) == VPK_ERR_ARG and pdf(ww=None) == VPK_ERR_ARG and pdf(p=None) == VPK_ERR_ARG and pdf(o=None) == VPK_ERR_ARG
    assert rt.lib.vpk_prior_params(rt.h, -1, P(maps), ctypes.c_double(0.1), P(wout)) == VPK_ERR_ARG
    assert rt.lib.vpk_prior_params(rt.h, 2, P(maps), ctypes.c_double(0.0), P(wout)) == VPK_ERR_ARG
    assert rt.lib.vpk_prior_params(rt.h, 2, None, ctypes.c_double(0.1), P(wout)) == VPK_ERR_ARG
    assert rt.lib.vpk_prior_params(rt.h, 2, P(maps), ctypes.c_double(0.1), None) == VPK_ERR_ARG
    assert rt.lib.vpk_prior_params(None, 2, P(maps), ctypes.c_double(0.1), P(wout)) == VPK_ERR_ARG
    # empty calls do nothing, whatever the pointers
    assert pdf(batch=0) == 0 and pdf(npts=0) == 0 and pdf(batch=0, m=None, o=None) == 0
    assert rt.lib.vpk_prior_params(rt.h, 0, None, ctypes.c_double(0.1), None) == 0
    rt.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (wout.cpu().numpy() == -7.0).all()
    # an empty mixture has density 0
    assert pdf(ncomp=0, m=None, ww=None) == 0
    rt.synchronize()
    assert (out.cpu().numpy() == 0.0).all()


def test_two_calls_give_the_same_bits():
    g = G()
    a = mixture(g["means"], g["weights"], g["sigma"], g["vecs"], want_angles=True)
    b = mixture(g["means"], g["weights"], g["sigma"], g["vecs"], want_angles=True)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)
    from vanishing_points_2017_amd import probability_functions as prob
    w1, w2 = prob.pdf_params_batch(g["maps"]).weights, prob.pdf_params_batch(g["maps"]).weights
    assert np.array_equal(w1.cpu().numpy(), w2.cpu().numpy(), equal_nan=True)
