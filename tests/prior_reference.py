"""What tests/test_prior_pdf.py (host build) and tests/test_gpu_prior_pdf.py (GPU) share: the reference's stored prior
densities (tests/golden/prior/prior_pdf.npz, written by scripts/make_prior_golden.py) and the bar they are held to.

The bar is derived, not measured.  The kernel adds the components in the reference's order, so a density differs from the
reference's only through its terms: each of up to 500 non-negative terms carries the exponential's own error (a few ulp,
tests/test_gpu_math.py) and |x| 2^-53 per rounding of its argument with |x| < 745 before it underflows -- together below
5e-13 relative.  So |got - ref| <= 1e-12 ref + 1e-300, NaN exactly where the reference has NaN, exact 0 where it has 0."""
import os

import numpy as np

from conftest import GOLDEN

PDF_RTOL = 1e-12
PDF_ATOL = 1e-300


def golden():
    return dict(np.load(os.path.join(GOLDEN, "prior", "prior_pdf.npz"), allow_pickle=False))


def check_pdf(got, ref, what=""):
    """Assert the bar on every element; returns the worst error as a fraction of the bar (for the test's printout)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN where the reference has none, or the reverse" % what
    assert np.all(got[ref == 0] == 0), "%s: not exactly 0 where the reference is" % what
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    frac = np.abs(got[ok] - ref[ok]) / (PDF_RTOL * ref[ok] + PDF_ATOL)
    assert frac.max() <= 1.0, "%s: %.3g x the bar at element %d" % (what, frac.max(), int(frac.argmax()))
    return float(frac.max())


def ulp_distance(a, b):
    """Distance in units of the last place between float64 arrays of equal sign pattern (NaN against NaN counts 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
    ia[ia < 0] = np.int64(-2 ** 63) - ia[ia < 0]        # order the negative numbers like the positive ones
    ib[ib < 0] = np.int64(-2 ** 63) - ib[ib < 0]
    d = np.abs(ia - ib)
    d[both_nan] = 0
    return d
