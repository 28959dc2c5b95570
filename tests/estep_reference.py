"""Extended-precision reference of the E-step's call surface -- calc_probabilities (probability_functions.py:99-120) with
the three distance measures calc_lvsq_angle (:157-176), calc_lvsq_dotprod (:150-154) and calc_lvsq_area (:179-209) -- its
per-element rounding bounds, the stored cases (tests/golden/estep/) and the generated ones, shared by
tests/test_estep_surface.py (CPU: the host build of csrc/estep_device.hpp) and tests/test_gpu_estep_surface.py (the kernel).

Every formula is restated from the reference's source in ``np.longdouble``.  A bound is never fitted to what a kernel
returns: it is the propagation of u = 2^-53 per rounded fp64 operation through the chain as csrc/estep_device.hpp writes it,
evaluated at the extended-precision values.

  angle     em_phase_reference.estep_reference, unchanged (19 u on cc = 1 - |cos|, see there)
  dotprod   lv = (l0 v0 + l1 v1) + l2 v2: three products and two sums, |d lv| <= 3 u sum |l_i v_i| in any order, fused or
            not; lvsq = lv^2: 2 |lv| d + d^2 + u lvsq
  area      b = |vl . (p1, 1)| with vl = (vy, -vx, vx my - vy mx) / |(vy, -vx)|: every term is a component of a unit vector
            (vx, vy one division each, the norm three operations of which the root halves two, the division by it: 6 u) times
            a coordinate (the midpoint: 1 u) and one product (1 u), and two sums of at most the terms' total S: d_b = 10 u S,
            taken as 12 u S for the second-order terms.  c = |lm - p2|: the midpoint's rounding u (|mx| + |my|) and four
            operations on c itself: d_c = u (|mx| + |my| + 4 c).  a = sqrt(c^2 - b^2) is evaluated at BOTH ends of the
            intervals of b and c (with the three roundings of the radicand, u (c^2 + b^2 + |r|)), as prior_reference does
            for asin: the bound stays valid where the radicand is 1e-8 of c^2.  t = a b^2 / c at both ends plus 3 u t;
            lvsq = t^2: 2 t d + d^2 + u lvsq.  Below a relative radicand of 1e-12 an element has no bound (the sign of the
            radicand is then a matter of rounding); no committed case may have one.
  p_lv, p_l, p_vl   em_phase_reference.estep_reference's scheme with the measure's own b_lvsq: the exponent moves by
            b_lvsq / (2 s) + 2 u a, exp is bounded by its values at both ends plus the device's 1 ulp and the resolution of
            an underflowing result, k2 is four operations, the product with p(v) one more and p(v)'s own bound; p_l sums M
            such terms in order; p_vl divides by it.
"""
import os

import numpy as np

import em_phase_reference as E

LD, U, PI, TINY, ld = E.LD, E.U, E.PI, E.TINY, E.ld

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "estep")
MEASURES = ("angle", "dotprod", "area")
MIN_REL_RADICAND = LD(1e-12)


# =============================================================================================================
# the three measures
# =============================================================================================================
def lvsq_angle(v, lp):
    """(lvsq, b_lvsq) (N, M): the expressions and the count of em_phase_reference.estep_reference."""
    lp_, vv = ld(lp), ld(np.asarray(v, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        vx, vy = vv[:, 0] / vv[:, 2], vv[:, 1] / vv[:, 2]
        lmx, lmy = LD(0.5) * (lp_[:, 0] + lp_[:, 2]), LD(0.5) * (lp_[:, 1] + lp_[:, 3])
        v2x, v2y = lp_[:, 0] - lp_[:, 2], lp_[:, 1] - lp_[:, 3]
        v1x, v1y = lmx[:, None] - vx[None, :], lmy[:, None] - vy[None, :]
        n1 = np.sqrt(v1x * v1x + v1y * v1y)
        n2 = np.sqrt(v2x * v2x + v2y * v2y)
        q = (v1x * v2x[:, None] + v1y * v2y[:, None]) / (n1 * n2[:, None])
        cc = 1 - np.abs(q)
        lvsq = cc * cc
        d_cc = U * (E.CC_UNIT_OPS + (np.abs(vx)[None, :] + np.abs(vy)[None, :] + np.abs(lmx)[:, None] + np.abs(lmy)[:, None]) / n1)
        b = 2 * np.abs(cc) * d_cc + d_cc * d_cc + U * lvsq
    return lvsq, b


def lvsq_dotprod(v, l):
    l_, vv = ld(l), ld(np.asarray(v, dtype=np.float64))
    terms = l_[:, None, :] * vv[None, :, :]
    lv = terms.sum(axis=2)
    d = 3 * U * np.abs(terms).sum(axis=2)
    lvsq = lv * lv
    return lvsq, 2 * np.abs(lv) * d + d * d + U * lvsq


def lvsq_area(v, lp):
    """(lvsq, b_lvsq, rel_radicand) (N, M).  Elements whose relative radicand is below MIN_REL_RADICAND get an infinite
    bound."""
    lp_, vv = ld(lp), ld(np.asarray(v, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        vx, vy = (vv[:, 0] / vv[:, 2])[None, :], (vv[:, 1] / vv[:, 2])[None, :]
        mx, my = (LD(0.5) * (lp_[:, 0] + lp_[:, 2]))[:, None], (LD(0.5) * (lp_[:, 1] + lp_[:, 3]))[:, None]
        p1x, p1y, p2x, p2y = (lp_[:, k][:, None] for k in range(4))
        nrm = np.sqrt(vx * vx + vy * vy)
        ux, uy = vy / nrm, -vx / nrm                                            # np.cross: (vy, -vx, vx my - vy mx) :200
        vl2 = (vx * my - vy * mx) / nrm
        bs = (ux * p1x + uy * p1y) + vl2
        b = np.abs(bs)                                                           # :203
        S = np.abs(ux * p1x) + np.abs(uy * p1y) + (np.abs(vx * my) + np.abs(vy * mx)) / nrm
        d_b = 12 * U * S
        dx, dy = mx - p2x, my - p2y
        c = np.sqrt(dx * dx + dy * dy) + 0 * b                                   # :204
        d_c = U * (np.abs(mx) + np.abs(my) + 4 * c)
        r = c * c - b * b
        d_r = U * (c * c + b * b + np.abs(r))
        a = np.sqrt(r)                                                           # :205
        b_lo, b_hi = np.maximum(b - d_b, 0), b + d_b
        c_lo, c_hi = np.maximum(c - d_c, 0), c + d_c
        a_hi = np.sqrt(np.maximum(c_hi * c_hi - b_lo * b_lo + d_r, 0))
        a_lo = np.sqrt(np.maximum(c_lo * c_lo - b_hi * b_hi - d_r, 0))
        d_a = np.maximum(a_hi - a, a - a_lo) + U * a
        t = a * (b * b) / c
        t_hi = (a + d_a) * (b_hi * b_hi) / c_lo
        t_lo = np.maximum(a - d_a, 0) * (b_lo * b_lo) / c_hi
        d_t = np.maximum(t_hi - t, t - t_lo) + 3 * U * t
        lvsq = t * t                                                             # :207
        bound = 2 * t * d_t + d_t * d_t + U * lvsq
        rel = r / (c * c)
        bound = np.where(rel < MIN_REL_RADICAND, LD(np.inf), bound)
    return lvsq, bound, rel


def lvsq_reference(measure, v, l, lp):
    if measure == "angle":
        return lvsq_angle(v, lp)
    if measure == "dotprod":
        return lvsq_dotprod(v, l)
    return lvsq_area(v, lp)[:2]


# =============================================================================================================
# the probabilities on top of a measure
# =============================================================================================================
def probabilities(lvsq, b_lvsq, s, p_v, b_pv):
    """calc_plv, p_l and calc_pvl in extended precision from (N, M) lvsq with its bound and p(v) (M,) with its bound: the
    scheme of em_phase_reference.estep_reference (:209-229 there), term for term."""
    p_v, b_pv = ld(p_v), ld(b_pv)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        sf = np.maximum(ld(s), LD(1e-200))                   # :139
        sf = np.where(np.isnan(sf), LD(1e-200), sf)          # `s[m] if s[m] > 1e-200 else 1e-200` replaces a NaN too
        a = lvsq / (2 * sf)[None, :]
        d_a = b_lvsq / (2 * sf)[None, :] + 2 * U * a
        e = np.exp(-a)
        e_hi = np.exp(-np.maximum(a - d_a, 0))
        e_lo = np.exp(-(a + d_a))
        d_e = np.maximum(e_hi - e, e - e_lo) + 2 * U * e + 2 * TINY
        k2 = 1 / np.sqrt(2 * PI * sf)
        scale = (k2 * p_v)[None, :]
        t = e * scale
        rel_scale = (5 * U + b_pv / p_v)[None, :]
        rel_scale = np.where(np.isfinite(rel_scale), rel_scale, 5 * U + 0 * rel_scale)      # p_v = 0: the term is 0
        d_t = d_e * np.abs(scale) * (1 + rel_scale) + np.abs(t) * rel_scale
        p_lv = e * k2[None, :]
        b_plv = d_e * k2[None, :] * (1 + 5 * U) + np.abs(p_lv) * 5 * U + TINY
        m_n = lvsq.shape[1]
        sum_t = t.sum(axis=1)
        d_pl = d_t.sum(axis=1) + m_n * U * np.abs(t).sum(axis=1)
        p_l = np.maximum(sum_t, LD(1e-12))                   # :117
        p_vl = (t / p_l[:, None]).T                          # :128
        b_pvl = ((d_t + np.abs(t) * (d_pl / p_l + 2 * U)[:, None]) / p_l[:, None]).T + TINY
    return {"s": sf, "p_lv": p_lv, "b_p_lv": b_plv, "p_l": p_l, "b_p_l": d_pl + TINY, "p_vl": p_vl, "b_p_vl": b_pvl}


def reference(measure, v, l, lp, s, p_v=None, pdfpar=None):
    """The whole call: p(v) from ``pdfpar`` = (means, weights, sigma) with prior_reference's bound, or ``p_v`` taken as
    exact fp64 input.  Dict of lvsq, p_lv (N, M), p_l (N), p_vl (M, N), s, p_v and b_<name>."""
    if pdfpar is not None:
        pv, b_pv, _ = E.prior_reference(pdfpar, np.asarray(v, dtype=np.float64))
    else:
        pv, b_pv = ld(p_v), np.zeros(np.shape(p_v), dtype=LD)
    lvsq, b = lvsq_reference(measure, v, l, lp)
    out = probabilities(lvsq, b, s, pv, b_pv)
    out.update(lvsq=lvsq, b_lvsq=b, p_v=pv, b_p_v=b_pv)
    return out


KEYS = ("lvsq", "p_lv", "p_l", "p_vl")


def check(out, ref, what, keys=KEYS):
    """NaN positions equal to the reference's and every finite element within its bound; returns {key: worst error / bound}."""
    worst = {}
    for k in keys:
        if out.get(k) is None:
            continue
        got = np.asarray(out[k], dtype=np.float64)
        want = ref[k]
        assert got.shape == want.shape, "%s: %s has shape %r, expected %r" % (what, k, got.shape, want.shape)
        want64 = want.astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want64)), "%s: NaN positions of %s differ" % (what, k)
        assert np.array_equal(np.isposinf(got), np.isposinf(want64)) and np.array_equal(np.isneginf(got), np.isneginf(want64)), \
            "%s: Inf positions of %s differ" % (what, k)
        r = E._ratio(np.abs(ld(got) - want), ref["b_" + k])
        worst[k] = r
        assert r <= 1.0, "%s: %s error / bound = %.3g" % (what, k, r)
    return worst


# =============================================================================================================
# cases
# =============================================================================================================
def golden_names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz"))


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def golden_pdfpar(g):
    return (g["means"], g["weights"], float(g["sigma"]))


# tiling: a workgroup covers 64 lines and stages 128 VPs at a time
SHAPE_N = (1, 63, 64, 65, 130)
SHAPE_M = (1, 2, 64, 65, 127, 128, 129)


def shapes():
    """Every N with three M and every M with at least two N; (130, 129) and (1, 1) among them."""
    out = []
    for i, n in enumerate(SHAPE_N):
        for j in range(3):
            out.append((n, SHAPE_M[(3 * i + 2 * j) % 7]))
    out += [(1, 1), (130, 129), (65, 128), (63, 127)]
    return sorted(set(out))


def case(n, m, seed=None):
    """lp (n, 4), l (n, 3), v (m, 3), s (m), p_v (m): a synthetic scene's segments against random VPs in front of the camera
    (|z| >= 0.05), the scene's own among them; variances of the measures' own sizes; p_v positive."""
    from vanishing_points_2017_amd import synth
    seed = 7000 * n + m if seed is None else seed
    rs = np.random.RandomState(seed)
    sc = synth.make_scene(seed, max(n, 12), 3)
    lp = np.ascontiguousarray(sc["lp"][:n], dtype=np.float64)
    l = np.cross(np.c_[lp[:, :2], np.ones(n)], np.c_[lp[:, 2:], np.ones(n)])
    l /= np.sqrt((l * l).sum(1))[:, None]
    v = rs.randn(m, 3)
    v[:, 2] = np.abs(v[:, 2]) + 0.05
    tv = np.asarray(sc["true_vps"], dtype=np.float64)
    tv = tv * np.where(tv[:, 2:3] < 0, -1.0, 1.0)
    tv = tv[tv[:, 2] > 1e-3]                                # (a VP at infinity makes every p_l of the call NaN: the goldens have one)
    k = min(m, tv.shape[0])
    if k:
        v[m - k:] = tv[:k]
    v /= np.sqrt((v * v).sum(1))[:, None]
    s = 10.0 ** rs.uniform(-6, -1, m)
    p_v = rs.uniform(0.05, 3.0, m)
    return {"lp": lp, "l": l, "v": v, "s": s, "p_v": p_v}
