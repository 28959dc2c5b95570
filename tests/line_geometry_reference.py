"""References of the stand-alone line geometry (vp_localisation.calc_lsim, line_rating_knn, lines_angles, line_length) and
the bars its tests hold an implementation to: tests/test_line_geometry.py (CPU: the host build of csrc/line_device.hpp)
and tests/test_gpu_line_geometry.py (the HIP kernels).  CPU only.

Two references, both restated from the reference's formulae (vp_localisation.py:34-108 and :700-776):

  extended   em_phase_reference.pairwise_reference generalised to the similarity's sigma and to the rating's sigma, k1 and
             k2, in np.longdouble, with the same ``clear`` mask: the rows whose k1-th and (k1+1)-th distances and whose k2-th
             and (k2+1)-th cosines differ by more than 1e-9 relative (two cosines tied at the clipped value 6.1e-17 do not
             count as a tie)
  float64    the four functions in plain NumPy float64

The bars are em_phase_reference.check_pairwise's: |lsim - ref| <= 1e-12 and |lscore - ref| <= 1e-12 (on clear rows) against
both references where the reference is finite, langle within 1e-13 of NumPy and within the extended reference's own bound,
llen within 1 ulp, the NaN / Inf pattern NumPy's, at most N // 100 rows of an image left out as not clear."""
import functools

import numpy as np

import em_phase_reference as E
from em_phase_reference import LD, PI, U, ld

SHAPES = (1, 2, 3, 7, 12, 64, 65, 129, 513)      # N < k2, N < k1, tile edges, special pairs from 129, several row blocks
RAGGED = (0, 1, 12, 129, 65)                     # one batch with an empty image
KNN = ((10, 3), (10, 4), (16, 5), (5, 1), (10, 10), (1, 1))
RATING_SIGMAS = (1.0, 0.3)
SIM_SIGMAS = (0.1, 1.0, 0.03)


@functools.lru_cache(maxsize=None)
def case(n):
    lp = E.pairwise_case(n) if n > 0 else np.zeros((0, 4))
    lp.setflags(write=False)
    return lp


def _pairs(lp, dtype):
    """Per pair: closest distance (:727-758), sharpened cosine (:715-724, f = 9); per line: its length (:761)."""
    lp_ = ld(lp) if dtype == LD else np.asarray(lp, dtype=np.float64)
    pi = PI if dtype == LD else np.pi
    x1, y1, x2, y2 = (lp_[:, k][:, None] for k in range(4))
    u1, w1, u2, w2 = (lp_[:, k][None, :] for k in range(4))
    d = np.minimum(np.minimum(E._seg_point_dist(x1, y1, x2, y2, u1, w1), E._seg_point_dist(x1, y1, x2, y2, u2, w2)),
                   np.minimum(E._seg_point_dist(u1, w1, u2, w2, x1, y1), E._seg_point_dist(u1, w1, u2, w2, x2, y2)))
    vx, vy = lp_[:, 0] - lp_[:, 2], lp_[:, 1] - lp_[:, 3]
    nrm = np.sqrt(vx * vx + vy * vy)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.abs((vx[:, None] * vx[None, :] + vy[:, None] * vy[None, :]) / (nrm[:, None] * nrm[None, :]))
        cos9 = np.cos(np.clip(9 * np.abs(np.arccos(np.clip(c, -1, 1))), -pi / 2, pi / 2))
    return d, cos9, vx, nrm


def _prox(d, nrm, sigma):
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        sg = d.dtype.type(sigma) * np.minimum(nrm[:, None], nrm[None, :])                       # :709
        return np.exp(-(d * d) / (2 * sg * sg))                                                 # :711


def _lsim(d, cos9, nrm, sigma):
    low = np.tril(cos9 * _prox(d, nrm, sigma), -1)                                              # :102-108
    return low + low.T                                                                          # :95-97


def _rating(d, cos9, nrm, k1, k2, sigma, want_clear):
    """line_rating_knn (:34-72).  Neighbours by (distance, index), the best cosines by argsort(...)[::-1] of a stable sort
    (NumPy's sort of up to 16 elements is an insertion sort)."""
    T = d.dtype.type
    n = d.shape[0]
    kk1, kk2 = min(k1, n), min(k2, n)                                                           # :40-41
    prox = _prox(d, nrm, sigma)
    dd = d.copy()
    np.fill_diagonal(dd, T(4))                                                                  # :82
    order = np.argsort(dd, axis=1, kind="stable")
    lscore = np.zeros(n, dtype=d.dtype)
    clear = np.ones(n, dtype=bool)

    def apart(a, b):
        return abs(a - b) > T(1e-9) * max(abs(a), abs(b))

    for i in range(n):
        if want_clear and n > kk1 and not apart(dd[i, order[i, kk1 - 1]], dd[i, order[i, kk1]]):
            clear[i] = False
        nn = order[i, :kk1]
        cs = cos9[i, nn]
        best = np.argsort(cs, kind="stable")[::-1]
        if want_clear and kk1 > kk2 and not apart(cs[best[kk2 - 1]], cs[best[kk2]]) and cs[best[kk2 - 1]] > T(1e-15):
            clear[i] = False
        acc = T(0)
        for j in nn[best[:kk2]]:
            acc += prox[i, j] * cos9[i, j]        # :65 measures the pair again: distance 0, not 4, for the line itself
        lscore[i] = acc / kk2                     # :70
    return lscore, clear


@functools.lru_cache(maxsize=None)
def _pairs_of(n, extended):
    return _pairs(case(n), LD if extended else np.float64)


@functools.lru_cache(maxsize=None)
def lsim_reference(n, sigma):
    """(extended, float64) similarity matrices of case(n)."""
    out = []
    for ext in (True, False):
        d, cos9, _, nrm = _pairs_of(n, ext)
        out.append(_lsim(d, cos9, nrm, sigma))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rating_reference(n, k1, k2, sigma):
    """(extended lscore, clear, float64 lscore) of case(n)."""
    d, cos9, _, nrm = _pairs_of(n, True)
    ext, clear = _rating(d, cos9, nrm, k1, k2, sigma, True)
    d, cos9, _, nrm = _pairs_of(n, False)
    f64, _ = _rating(d, cos9, nrm, k1, k2, sigma, False)
    return ext, clear, f64


@functools.lru_cache(maxsize=None)
def angle_reference(n):
    """lines_angles (:765-776) and line_length (:761): extended angle, its bound (pairwise_reference's: acos over an
    argument with three rounded operations in it, x +- 4 u, plus 2 u pi), float64 angle, extended and float64 lengths."""
    _, _, vx, nrm = _pairs_of(n, True)
    with np.errstate(divide="ignore", invalid="ignore"):
        xa = np.clip(vx / nrm, -1, 1)
        phi = np.abs(np.arccos(xa))
        lo = np.abs(np.arccos(np.clip(xa + 4 * U, -1, 1)))
        hi = np.abs(np.arccos(np.clip(xa - 4 * U, -1, 1)))
    ext = np.where(phi > PI / 2, PI - phi, phi)
    bound = np.maximum(phi - lo, hi - phi) + 2 * U * PI
    lp = case(n)
    f64 = np.zeros(n)
    ln64 = np.zeros(n)
    for i in range(n):
        v = np.array([lp[i, 0] - lp[i, 2], lp[i, 1] - lp[i, 3]])
        ln64[i] = np.linalg.norm(v, ord=2)
        v = v / np.linalg.norm(v)
        p = np.abs(np.arccos(np.clip(v[0], -1, 1)))
        f64[i] = np.pi - p if p > np.pi / 2 else p
    return ext, bound, f64, nrm, ln64


# ---- the bars -----------------------------------------------------------------------------------------------------------
def _bar(name, err, bound, n):
    r = E._ratio(err, bound)
    print("%-28s N = %-4d error / bar = %.3g" % (name, n, r))
    assert r <= 1.0, "%s (N = %d): error / bar = %.3g" % (name, n, r)
    return r


def check_lsim(lsim, n, sigma):
    ext, f64 = lsim_reference(n, sigma)
    assert lsim.shape == (n, n) and lsim.dtype == np.float64
    assert E.same_pattern(lsim, f64), "NaN / Inf pattern of lsim differs from NumPy's"
    assert np.array_equal(lsim, lsim.T, equal_nan=True), "lsim is not symmetric bit for bit"
    assert (np.diagonal(lsim) == 0).all() and not np.signbit(np.diagonal(lsim)).any()
    fin = np.isfinite(f64)
    return max(_bar("lsim s=%g" % sigma, np.abs(lsim - f64)[fin], LD(1e-12), n),
               _bar("lsim s=%g ext" % sigma, np.abs(ld(lsim) - ext)[fin], LD(1e-12), n))


def check_lscore(lscore, n, k1, k2, sigma):
    ext, clear, f64 = rating_reference(n, k1, k2, sigma)
    assert lscore.shape == (n,) and lscore.dtype == np.float64
    assert E.same_pattern(lscore, f64), "NaN / Inf pattern of lscore differs from NumPy's"
    assert (~clear).sum() <= n // 100, "more than N // 100 rows are left out of the score comparison: %d of %d" % ((~clear).sum(), n)
    fin = np.isfinite(f64) & clear
    tag = "lscore k=%d,%d s=%g" % (k1, k2, sigma)
    return max(_bar(tag, np.abs(lscore - f64)[fin], LD(1e-12), n), _bar(tag + " ext", np.abs(ld(lscore) - ext)[fin], LD(1e-12), n))


def ulp_distance(a, b):
    a, b = (np.ascontiguousarray(x, dtype=np.float64).view(np.int64) for x in (a, b))     # positive finite values only
    return np.abs(a - b)


def check_angles(langle, llen, n):
    ext, bound, f64, len_ext, len64 = angle_reference(n)
    assert langle.shape == llen.shape == (n,)
    assert E.same_pattern(langle, f64) and E.same_pattern(llen, len64), "NaN / Inf pattern differs from NumPy's"
    fin = np.isfinite(f64)
    r = max(_bar("langle", np.abs(langle - f64)[fin], LD(1e-13), n),
            _bar("langle ext", np.abs(ld(langle) - ext)[fin], np.maximum(bound[fin], 0), n))
    assert (llen > 0).all()
    worst = max(int(ulp_distance(llen, len64).max()), int(ulp_distance(llen, len_ext.astype(np.float64)).max())) if n else 0
    print("%-28s N = %-4d %d ulp" % ("llen", n, worst))
    assert worst <= 1, "line lengths %d ulp from the reference" % worst
    return r
