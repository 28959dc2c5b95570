"""The prior's device code (csrc/prior_device.hpp) compiled for the host by tests/hostsim/sim_prior.cpp and run serially,
and the host side of probability_functions, against the reference's stored output (tests/golden/prior/prior_pdf.npz).  The
kernels themselves: tests/test_gpu_prior_pdf.py."""
import ctypes

import numpy as np
import pytest

import prior_reference as R
from hostsim import hostbuild


@pytest.fixture(scope="module")
def sim():
    lib = hostbuild.load("prior")
    D, F, I = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.c_int
    lib.sim_prior_params.argtypes = [I, F, ctypes.c_double, F]
    lib.sim_mixture_pdf.argtypes = [I, I, D, I, D, ctypes.c_double, I, D, I, I, D, D]
    return lib


@pytest.fixture(scope="module")
def g():
    return R.golden()


def _d(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None


def _mixture(sim, means, weights, sigma, pts, angles=False):
    means, weights, pts = (np.ascontiguousarray(a, dtype=np.float64) for a in (means, weights, pts))
    batch, ncomp = weights.shape
    npts, dim = pts.shape[-2:]
    pdf = np.full((batch, npts), -1.0)
    ang = np.full((batch, npts, 2), -1.0) if angles else None
    sim.sim_mixture_pdf(batch, ncomp, _d(means), int(means.ndim == 2), _d(weights), float(sigma), npts, _d(pts), dim,
                        int(pts.ndim == 2), _d(ang), _d(pdf))
    return ang, pdf


def test_host_build_weights_are_the_references(sim, g):
    maps = np.ascontiguousarray(g["maps"].reshape(-1, 400))
    keep = maps.copy()
    w = np.full_like(maps, -1.0)
    F = ctypes.POINTER(ctypes.c_float)
    sim.sim_prior_params(maps.shape[0], maps.ctypes.data_as(F), float(g["sigma"]), w.ctypes.data_as(F))
    assert np.array_equal(maps, keep)
    assert w.dtype == g["weights"].dtype == np.float32
    assert np.array_equal(w, g["weights"], equal_nan=True)
    assert np.isnan(g["weights"][5]).all() and [(x > 0).sum() for x in g["weights"]] == [100, 100, 100, 7, 100, 0]


def test_host_build_densities_meet_the_bar(sim, g):
    """Every stored map at every stored point, the points shared by the maps; and given per image (each image another
    rotation of the list)."""
    _, pdf = _mixture(sim, g["means"], g["weights"], g["sigma"], g["pts"])
    print("worst error / bar %.3g" % R.check_pdf(pdf, g["pdf"], "shared points"))
    rolled = np.stack([np.roll(g["pts"], 37 * b, axis=0) for b in range(6)])
    _, pdf = _mixture(sim, g["means"], g["weights"], g["sigma"], rolled)
    R.check_pdf(pdf, np.stack([np.roll(g["pdf"][b], 37 * b) for b in range(6)]), "points per image")


def test_host_build_vector_form(sim, g):
    """pts_dim = 3: calc_angles in front of the density.  The host build's asin / cos are libm's and NumPy has its own, so
    the angles are held to 4 ulp (asin of an argument one ulp off, next to each function's own last bit), as on the GPU."""
    ang, pdf = _mixture(sim, g["means"], g["weights"], g["sigma"], g["vecs"], angles=True)
    ulp = R.ulp_distance(ang, np.broadcast_to(g["angles"], ang.shape))
    print("angles: worst %d ulp" % ulp.max())
    assert ulp.max() <= 4
    print("worst error / bar %.3g" % R.check_pdf(pdf, g["pdf_vec"], "vectors"))


def test_host_build_arbitrary_mixture(sim, g):
    """130 components (two LDS chunks) with means of their own per image, weights 0, negative and NaN among them."""
    means = np.stack([g["arb_means"], g["arb_means"]])
    _, pdf = _mixture(sim, means, np.stack([g["arb_weights"]] * 2), g["arb_sigma"], g["pts"][:70])
    R.check_pdf(pdf, np.stack([g["arb_pdf"]] * 2), "arbitrary mixture")


def test_calc_angles_is_the_references(g):
    from vanishing_points_2017_amd import probability_functions as prob
    with np.errstate(all="ignore"):
        got = prob.calc_angles(g["vecs"].shape[0], g["vecs"])
    assert np.array_equal(got, g["angles"], equal_nan=True)
    nan = prob.calc_angles(1, np.array([[np.nan, 0.5, 0.1]]))
    assert np.isnan(nan[0, 0]) and nan[0, 1] == np.arcsin(0.5)


def test_means_and_sigma_are_the_references(g):
    from vanishing_points_2017_amd import probability_functions as prob
    assert np.array_equal(prob._grid_means(), g["means"])
    assert prob._sigma(1.282) == float(g["sigma"])
    assert prob._sigma(1.0) == np.pi / 20.0
    with pytest.raises(ValueError):
        prob.pdf_params(np.zeros((20, 21), dtype=np.float32))
    with pytest.raises(ValueError):
        prob.pdf_params_batch(np.zeros((3, 10, 10), dtype=np.float32))


def test_reference_names_and_host_helpers():
    from vanishing_points_2017_amd import probability_functions as prob
    for name in ("PDFParams", "PDF", "pdf_params", "calc_pdf", "calc_pdf_grid", "calc_angles", "pdf_grid",
                 "vp_is_within_image", "pdf_params_batch", "calc_pdf_batch", "vp_prior_batch", "pdf_grid_batch"):
        assert hasattr(prob, name), name
    assert prob.vp_is_within_image(np.array([1.0, -1.9, 1.0])) is True
    assert prob.vp_is_within_image(np.array([2.0, 0.0, 1.0])) is False
    assert prob.vp_is_within_image(np.array([0.5, 0.5, 0.2])) is False
    X, Y = prob._grid_xy(8)
    assert X.shape == Y.shape == (8, 8) and X[0, 0] == -np.pi / 2 and np.array_equal(X, Y.T)
