"""Extended-precision references of the EM's phases, their first-order error bounds, and the shared case generators of
tests/test_em_phases.py (CPU: the host build of the device source and the float64 oracle) and
tests/test_gpu_em_phases.py (the HIP kernels).  CPU only.

Every formula is restated from the reference's source in ``np.longdouble`` (x87 extended, 64-bit significand):

  E-step      probability_functions.py:99-120 (calc_probabilities), :122-129 (calc_pvl), :131-147 (calc_plv),
              :157-176 (calc_lvsq_angle), with calc_angles :252-259 and calc_pdf :8-40 for the prior
  pairwise    vp_localisation.py:34-84 (line_rating_knn), :87-108 (calc_lsim) with the segment geometry of :700-776
  initial VPs vp_localisation.py:111-165 (find_initial_vps) -- integer work, taken from oracle.em_numpy
  M-step      vp_localisation.py:294-317 (soft), :353-392 (hard), :453-479 (calc_new_vanishing_point)
  counts      vp_localisation.py:482-512 (calc_vp_line_counts)

A bound below is never fitted to what a kernel returns: it is the first-order propagation of u = 2^-53 per rounded fp64
operation through the chain as csrc/em_device.hpp writes it, evaluated at the extended-precision values.  The float64
oracle (oracle/em_numpy.py, LAPACK for the null vector) has to meet every one of them on every input generated here:
tests/test_em_phases.py checks that without a GPU.
"""
import numpy as np

LD = np.longdouble
# No skip: a skipped module would hide every test that imports it.
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble has no 64-bit significand here: the phase references need one"

U = LD(2.0) ** -53            # unit roundoff of fp64
PI = LD(np.pi) + LD(1.2246467991473532e-16)     # pi to extended precision (fp64 pi + its residual)
TINY = LD(2.0) ** -1074       # fp64's smallest subnormal: the resolution of an underflowing exp


def ld(a):
    """fp64 data (or values already extended) as longdouble."""
    a = np.asarray(a)
    return a if a.dtype == LD else a.astype(np.float64).astype(LD)


# =============================================================================================================
# null vector: one-sided Jacobi SVD in extended precision (numpy.linalg has no longdouble SVD)
# =============================================================================================================
def jacobi_svd(a, sweeps=60):
    """Singular values (descending) and right singular vectors (columns of V, same order) of the n x 3 matrix ``a`` by
    one-sided (Hestenes) Jacobi in longdouble: columns of A V are rotated pairwise until they are orthogonal to working
    precision.  Relative accuracy of the small singular values and vectors is the reason for the one-sided form."""
    w = np.array(ld(a), dtype=LD).reshape(-1, 3)
    v = np.eye(3, dtype=LD)
    eps = np.finfo(LD).eps
    for _ in range(sweeps):
        rotated = False
        for p in range(2):
            for q in range(p + 1, 3):
                alpha = np.dot(w[:, p], w[:, p])
                beta = np.dot(w[:, q], w[:, q])
                gamma = np.dot(w[:, p], w[:, q])
                if gamma == 0 or abs(gamma) <= eps * np.sqrt(alpha * beta):
                    continue
                rotated = True
                zeta = (beta - alpha) / (2 * gamma)
                t = (LD(1) if zeta >= 0 else LD(-1)) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                wp, wq = w[:, p].copy(), w[:, q].copy()
                w[:, p], w[:, q] = c * wp - s * wq, s * wp + c * wq
                vp, vq = v[:, p].copy(), v[:, q].copy()
                v[:, p], v[:, q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break
    sv = np.sqrt((w * w).sum(axis=0))
    order = np.argsort(-sv, kind="stable")
    return sv[order], v[:, order]


def c_of_n(n):
    """Rounding-error constant of the null vector and of its residual for n rows: n for the summation of n products in
    any order (gamma_n = n u), plus 32 for the fixed work per row and per solve -- the row weight w / max w (1), the
    row rotated into the current basis (5 per component), its products (2), and the 3 x 3 Jacobi eigen-solve and basis
    update (a few u of the matrix norm each)."""
    return LD(n + 32)


def null_vector_reference(l, r):
    """Third right singular vector of diag(r) l (vp_localisation.py:462-474) in extended precision, normalised and with
    the sign of its z component, the singular values, and the bounds of the issue's section "Bars":
      vec_bound  c(N) u s1 / (s2 - s3); where pass 0 of group_null_vector may leave without refinement
                 (s2^2 - s3^2 > 1e-3 s1^2, tested with 10 % slack on both sides) the normal-equations term
                 c(N) u s1^2 / (s2^2 - s3^2) instead -- the larger of the two where both may apply
      res_bound  s3 + c(N) u s1: |diag(r) l vp| of any backward-stable null vector, no condition number in it"""
    a = ld(r)[:, None] * ld(l)
    sv, v = jacobi_svd(a)
    if a.shape[0] < 3:
        sv = np.concatenate([sv, np.zeros(3 - a.shape[0], dtype=LD)])[:3]
    vp = v[:, 2] / np.sqrt(np.dot(v[:, 2], v[:, 2]))
    vp = vp * np.sign(vp[2])
    c = c_of_n(a.shape[0])
    s1, s2, s3 = sv[0], sv[1], sv[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        refined = c * U * s1 / (s2 - s3)
        normal = c * U * s1 * s1 / (s2 * s2 - s3 * s3)
    gap2 = s2 * s2 - s3 * s3
    if gap2 > LD(1.1e-3) * s1 * s1:
        vec = normal
    elif gap2 < LD(0.9e-3) * s1 * s1:
        vec = refined
    else:
        vec = max(normal, refined)
    if not np.isfinite(vec):
        vec = LD(np.inf)
    return {"vp": vp, "sv": sv, "vec_bound": vec, "res_bound": s3 + c * U * s1}


def residual(l, r, vp):
    """|diag(r) l vp| in extended precision."""
    y = (ld(r)[:, None] * ld(l)) @ ld(vp)
    return np.sqrt(np.dot(y, y))


# =============================================================================================================
# E-step
# =============================================================================================================
def prior_reference(pdfpar, v):
    """p(v) (calc_angles :252-259, calc_pdf :8-40) in extended precision with its bound.  alpha and beta carry the
    rounding of asin / cos / the division through the conditioning of asin, 1 / sqrt(1 - x^2), taken as an INTERVAL
    (asin evaluated at both ends of the argument's error interval) so that it stays valid next to the poles, where
    the first-order term has no meaning; p(v) then moves by |dp/dalpha| d_alpha + |dp/dbeta| d_beta, plus the rounding
    of the sum itself: about 110 u relative for 100 positive components summed by 16 lanes, and 8 u |d k| relative per
    exponential for its argument (six rounded operations) and the device's exp (1 ulp = 2 u)."""
    means, weights, sigma = pdfpar
    v = ld(v)
    sigma = LD(sigma)
    k = LD(-0.5) / (sigma * sigma)
    m_n = v.shape[0]
    p = np.zeros(m_n, dtype=LD)
    bound = np.zeros(m_n, dtype=LD)
    ang = np.zeros((m_n, 2), dtype=LD)
    comps = np.nonzero(np.asarray(weights) > 0)[0]
    for m in range(m_n):
        beta = np.arcsin(v[m, 1])
        cb = np.cos(beta)
        with np.errstate(divide="ignore", invalid="ignore"):
            inner = v[m, 0] / cb
        ang[m] = (np.nan, beta)
        if not np.isfinite(inner):
            p[m] = np.nan
            bound[m] = np.inf
            continue
        inner_c = min(max(inner, LD(-1)), LD(1))
        alpha = np.arcsin(inner_c)
        ang[m, 0] = alpha
        d_beta = 2 * U * abs(beta) + TINY
        d_inner = abs(inner) * (abs(np.tan(beta)) * d_beta + 4 * U)
        hi = np.arcsin(min(inner_c + d_inner, LD(1)))
        lo = np.arcsin(max(inner_c - d_inner, LD(-1)))
        d_alpha = max(hi - alpha, alpha - lo) + 2 * U * abs(alpha)
        acc = LD(0); ga = LD(0); gb = LD(0); rnd = LD(0)
        for q in comps:
            ma, mb, wq = LD(means[q, 0]), LD(means[q, 1]), LD(weights[q])
            terms = ((alpha - ma, beta - mb, 1), (alpha - ma + PI, beta + mb, 1), (alpha - ma - PI, beta + mb, 1),
                     (alpha + ma, beta - mb - PI, 2))            # the fifth term duplicates the fourth (:25-26)
            for da, db, mult in terms:
                d = da * da + db * db
                e = np.exp(d * k) * mult * wq
                acc += e
                ga += e * 2 * k * da
                gb += e * 2 * k * db
                rnd += e * (8 * abs(d * k) + 110) * U
        p[m] = acc
        # second-order slack of the interval step: the prior's curvature is bounded by 2 |k| p (1 + 2 |k| d^2)
        bound[m] = abs(ga) * d_alpha + abs(gb) * d_beta + rnd + 4 * abs(k) * acc * (d_alpha * d_alpha + d_beta * d_beta) * 40
    return p, bound, ang


# Rounded fp64 operations in the chain from the inputs to cc = 1 - |q| as line_geometry_setup / estep write it:
#   with unit weight (each moves cc by at most u, because |q| <= 1): v1x, v1y (2), v2x, v2y (2), dot2 (2),
#   n1 = sqrt(fma(.,., .*.)) (3), n2 (3), n1 * n2 (1), the division (1), 1 - |q| (1)                      = 15
#   with the weight |input| / n1 (they move the DIRECTION of v1): vx = x0 / x2, vy = x1 / x2 (2), the midpoint
#   additions lmx, lmy (2)                                                                                 =  4
CC_UNIT_OPS = 15
CC_WEIGHTED_OPS = 4


def estep_reference(pdfpar, v, lp, s):
    """calc_probabilities in extended precision: dict of p_v, lvsq (N,M), p_lv (N,M), p_l (N), p_vl (M,N), s (floored),
    and per-element bounds b_pv, b_lvsq, b_pl, b_pvl.

    cc = 1 - |cos|: C = 15 rounded operations move it by at most u each and 4 more (the VP's image point and the
    line's midpoint) by u |input| / n1 -- 19 in all (CC_UNIT_OPS, CC_WEIGHTED_OPS above).  lvsq = cc^2 adds one.
    The exponent a = lvsq / (2 s) moves by d_lvsq / (2 s) + 2 u a, and exp(-a) is bounded by its values at both ends of
    that interval (first order where the interval is short, still valid where it is not) plus the device's exp (1 ulp,
    tests/test_gpu_math.py) and the resolution of an underflowing result; k2 = 1 / sqrt(2 pi s) is four operations,
    the product with p(v) one more and p(v)'s own bound.  p_l sums M such terms in order; p_vl divides by it."""
    v64 = np.asarray(v, dtype=np.float64)
    lp_ = ld(lp)
    vv = ld(v64)
    p_v, b_pv, _ = prior_reference(pdfpar, v64)
    with np.errstate(divide="ignore", invalid="ignore"):
        vx = vv[:, 0] / vv[:, 2]
        vy = vv[:, 1] / vv[:, 2]
        lmx = LD(0.5) * (lp_[:, 0] + lp_[:, 2])
        lmy = LD(0.5) * (lp_[:, 1] + lp_[:, 3])
        v2x = lp_[:, 0] - lp_[:, 2]
        v2y = lp_[:, 1] - lp_[:, 3]
        v1x = lmx[:, None] - vx[None, :]
        v1y = lmy[:, None] - vy[None, :]
        n1 = np.sqrt(v1x * v1x + v1y * v1y)
        n2 = np.sqrt(v2x * v2x + v2y * v2y)
        q = (v1x * v2x[:, None] + v1y * v2y[:, None]) / (n1 * n2[:, None])
        cc = 1 - np.abs(q)
        lvsq = cc * cc
        d_cc = U * (CC_UNIT_OPS + (np.abs(vx)[None, :] + np.abs(vy)[None, :] + np.abs(lmx)[:, None] + np.abs(lmy)[:, None]) / n1)
        b_lvsq = 2 * np.abs(cc) * d_cc + d_cc * d_cc + U * lvsq
        sf = np.maximum(ld(s), LD(1e-200))                   # :139
        a = lvsq / (2 * sf)[None, :]
        d_a = b_lvsq / (2 * sf)[None, :] + 2 * U * a
        e = np.exp(-a)
        e_hi = np.exp(-np.maximum(a - d_a, 0))
        e_lo = np.exp(-(a + d_a))
        d_e = np.maximum(e_hi - e, e - e_lo) + 2 * U * e + 2 * TINY
        k2 = 1 / np.sqrt(2 * PI * sf)
        scale = (k2 * p_v)[None, :]
        t = e * scale                                        # p_lv * p_v, the term of p_l (:116)
        rel_scale = (5 * U + b_pv / p_v)[None, :]
        d_t = d_e * np.abs(scale) * (1 + rel_scale) + np.abs(t) * rel_scale
        p_lv = e * k2[None, :]
        m_n = vv.shape[0]
        sum_t = t.sum(axis=1)
        d_pl = d_t.sum(axis=1) + m_n * U * np.abs(t).sum(axis=1)
        p_l = np.maximum(sum_t, LD(1e-12))                   # :117
        p_vl = (t / p_l[:, None]).T                          # :128
        b_pvl = ((d_t + np.abs(t) * (d_pl / p_l + 2 * U)[:, None]) / p_l[:, None]).T + TINY
    return {"p_v": p_v, "b_pv": b_pv, "lvsq": lvsq, "b_lvsq": b_lvsq, "p_lv": p_lv, "p_l": p_l, "b_pl": d_pl + TINY,
            "p_vl": p_vl, "b_pvl": b_pvl, "s": sf}


# =============================================================================================================
# pairwise: calc_lsim, line_rating_knn, lines_angles
# =============================================================================================================
def _seg_point_dist(ax, ay, bx, by, px, py):
    """vp_localisation.py:743-758 (the reference squares the norm of b - a, :747: the same number here)."""
    dx, dy = bx - ax, by - ay
    with np.errstate(divide="ignore", invalid="ignore"):
        param = ((px - ax) * dx + (py - ay) * dy) / (dx * dx + dy * dy)
    cx = np.where(param < 0, ax, np.where(param > 1, bx, ax + param * dx))
    cy = np.where(param < 0, ay, np.where(param > 1, by, ay + param * dy))
    ex, ey = cx - px, cy - py
    return np.sqrt(ex * ex + ey * ey)


def pairwise_reference(lp, k1=10, k2=4):
    """calc_lsim (sigma = 1, vp_localisation.py:178), line_rating_knn (k2 = 4 at the call site :230) and lines_angles in
    extended precision.  Returns lsim, lscore, langle, the bound of langle (acos is evaluated on an argument with three
    rounded operations in it: the interval of acos over x +- 4 u, plus 2 u pi -- next to a horizontal line the
    conditioning of acos, 1 / sqrt(1 - x^2), is all there is), and ``clear``: the rows whose k1-th and (k1+1)-th
    distances and whose k2-th and (k2+1)-th cosines differ by more than 1e-9 relative -- the rows on which the score is
    a function of the data and not of how a tie falls."""  # noqa
    lp_ = ld(lp)
    n = lp_.shape[0]
    x1, y1, x2, y2 = (lp_[:, k][:, None] for k in range(4))
    u1, w1, u2, w2 = (lp_[:, k][None, :] for k in range(4))
    d = np.minimum(np.minimum(_seg_point_dist(x1, y1, x2, y2, u1, w1), _seg_point_dist(x1, y1, x2, y2, u2, w2)),
                   np.minimum(_seg_point_dist(u1, w1, u2, w2, x1, y1), _seg_point_dist(u1, w1, u2, w2, x2, y2)))
    vx, vy = lp_[:, 0] - lp_[:, 2], lp_[:, 1] - lp_[:, 3]
    nrm = np.sqrt(vx * vx + vy * vy)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.abs((vx[:, None] * vx[None, :] + vy[:, None] * vy[None, :]) / (nrm[:, None] * nrm[None, :]))
        cos9 = np.cos(np.clip(9 * np.abs(np.arccos(np.clip(c, -1, 1))), -PI / 2, PI / 2))       # :715-724
        sg = np.minimum(nrm[:, None], nrm[None, :])
        prox = np.exp(-(d * d) / (2 * sg * sg))                                                 # :708-712
    sim = cos9 * prox
    low = np.tril(sim, -1)
    lsim = low + low.T
    kk1, kk2 = min(k1, n), min(k2, n)
    dd = d.copy()
    np.fill_diagonal(dd, LD(4))                                                                 # :82
    lscore = np.zeros(n, dtype=LD)
    clear = np.ones(n, dtype=bool)

    def apart(a, b):
        return abs(a - b) > LD(1e-9) * max(abs(a), abs(b))

    for i in range(n):
        order = np.argsort(dd[i], kind="stable")
        if n > kk1 and not apart(dd[i, order[kk1 - 1]], dd[i, order[kk1]]):
            clear[i] = False
        nn = order[:kk1]
        cs = cos9[i, nn]
        best = np.argsort(cs, kind="stable")[::-1]
        # (two cosines tied at the clipped value cos(pi / 2) = 6.1e-17 do not count: whichever of them is taken, the score
        #  moves by less than 1e-16, so such a row stays in the comparison)
        if kk1 > kk2 and not apart(cs[best[kk2 - 1]], cs[best[kk2]]) and cs[best[kk2 - 1]] > LD(1e-15):
            clear[i] = False
        acc = LD(0)
        for j in nn[best[:kk2]]:
            acc += prox[i, j] * cos9[i, j]        # :65 recomputes the pair's distance: 0, not 4, for the line itself
        lscore[i] = acc / kk2
    with np.errstate(divide="ignore", invalid="ignore"):
        xa = np.clip(vx / nrm, -1, 1)
        phi = np.abs(np.arccos(xa))
        lo = np.abs(np.arccos(np.clip(xa + 4 * U, -1, 1)))
        hi = np.abs(np.arccos(np.clip(xa - 4 * U, -1, 1)))
    langle = np.where(phi > PI / 2, PI - phi, phi)
    b_angle = np.maximum(phi - lo, hi - phi) + 2 * U * PI
    return {"lsim": lsim, "lscore": lscore, "langle": langle, "b_langle": b_angle, "clear": clear}


# =============================================================================================================
# M-step: the whole iteration of one VP (vp_localisation.py:284-317 soft, :353-392 hard)
# =============================================================================================================
def mstep_reference(l, w, lvsq, p_vl, cur, assoc=None, max_stdd=1e-6, s_thresh=1e-200):
    """Per VP a dict: kind ('skip' = the hard mode's `continue`, 'none' = newVP is None, 'one' = one selected row,
    'svd'), and for 'one' / 'svd': the extended-precision s (clamped) with its relative bound, the null vector with its
    bounds (null_vector_reference), err with its bound and the margins of the discrete decisions.

    Variance (:301-307): both sums have non-negative terms, (N + 1) u relative each in any order; each log is 1 ulp of
    its value, the difference and exp one more each: rel_s = (2 N + 8) u + 2 u (|ln sv| + |ln sp|).  err = acos(min(|cur .
    vp|, 1)) (:312): an interval of acos over d +- (|d_vp| + 4 u), plus 2 u pi."""
    l_ = ld(l)
    m_n, n = np.asarray(w).shape
    out = []
    for m in range(m_n):
        sel = np.ones(n, dtype=bool) if assoc is None else (np.asarray(assoc) == m)
        if assoc is not None and not sel.any():
            out.append({"kind": "skip"})
            continue
        wm = np.asarray(w[m], dtype=np.float64)[sel]
        if np.isnan(wm).any() or wm.size == 0 or np.nanmax(wm) == 0:
            out.append({"kind": "none"})                      # :456-460, LinAlgError on a NaN -> None
            continue
        wmax = np.max(wm)
        r = np.zeros(n, dtype=LD)
        r[sel] = ld(wm) / LD(wmax)
        rec = {"kind": "one" if sel.sum() == 1 else "svd", "r": r.astype(np.float64), "sel": sel}
        rec.update(null_vector_reference(l_, r))
        sv_ = (ld(lvsq[m]) * ld(p_vl[m])).sum()
        sp_ = ld(p_vl[m]).sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            s_raw = sv_ / sp_ if not (sv_ == 0 and sp_ == 0) else LD(np.nan)
            rel_s = (2 * n + 8) * U + 2 * U * (abs(np.log(sv_)) + abs(np.log(sp_)))
        s = s_raw
        if not np.isnan(s):
            s = min(s, LD(max_stdd))
            if assoc is None:
                s = max(s, LD(s_thresh))
        rec.update(s=s, s_raw=s_raw, rel_s=rel_s)
        out.append(rec)
    return out


def err_reference(cur, vp, d_vp):
    """err (:312) in extended precision and its interval bound for a VP known to within d_vp."""
    d = abs(np.dot(ld(cur), ld(vp)))
    dd = LD(d_vp) + 4 * U
    e = np.arccos(min(d, LD(1)))
    lo = np.arccos(min(d + dd, LD(1)))
    hi = np.arccos(max(min(d - dd, LD(1)), LD(0)))
    return e, max(e - lo, hi - e) + 2 * U * PI


# =============================================================================================================
# shared case generators: both test files see identical inputs
# =============================================================================================================
SIGMAS = (1e-300, 1e-12, 1.2e-7, 1e-4, 1e-2)


def _scene(seed, n):
    from vanishing_points_2017_amd import synth
    sc = synth.make_scene(seed, max(n, 12), 3)
    return sc


# Every N meets an M < 8, an M with M % 4 != 0, M = 32 and M = 33; together the pairs cover all eleven M.
ESTEP_N = (1, 2, 7, 64, 65, 128, 129, 256, 257, 513)
ESTEP_M = (1, 2, 3, 5, 8, 9, 31, 32, 33, 40, 64)


def estep_shapes():
    out = []
    for i, n in enumerate(ESTEP_N):
        extra = [ESTEP_M[(2 * i) % 11], ESTEP_M[(2 * i + 1) % 11], ESTEP_M[i % 4]]     # the last is one of 1, 2, 3, 5: M < 8, M % 4 != 0
        for m in sorted(set(extra + [32, 33])):
            out.append((n, m))
    return out


def special_vps():
    y = 1 - 1e-6
    c = np.sqrt(1 - y * y)
    return np.array([[0.0, 0.0, 1.0],                      # the image centre
                     [0.6, 0.8, 0.0],                      # z = 0: a point at infinity (vx, vy infinite)
                     [0.6 * c, y, 0.8 * c],                # |y| = 1 - 1e-6: next to asin's pole
                     [-0.6 * c, -y, 0.8 * c]])


def estep_case(n, m, midpoint_line=True):
    """lp (n,4), cnn (20,20) f32, v (m,3), s (m): a synthetic scene's first n segments and m VPs; the special lines and
    VPs of the issue are placed from the front, so the small shapes have them too."""
    seed = 1000 * n + m
    rs = np.random.RandomState(seed)
    sc = _scene(seed, n)
    lp = sc["lp"][:n].copy()
    v = rs.randn(m, 3)
    v[:, 2] = np.abs(v[:, 2]) + 0.05
    tv = np.asarray(sc["true_vps"], dtype=np.float64)
    k = min(m, tv.shape[0])
    v[m - k:] = tv[:k]                                      # the scene's own VPs: lines that point at them (cc ~ 0)
    v /= np.sqrt((v * v).sum(1))[:, None]
    sp = special_vps()
    # z = 0 makes lvsq NaN for every line, so p_l and with it every p_vl of the call: only a quarter of the calls have it
    if m >= 5:
        keep = v[1].copy()
        v[:4] = sp
        if (n + m) % 4:
            v[1] = keep
    elif m >= 2:
        v[0] = sp[(n + m) % 4]
    if n >= 7:
        vx, vy = v[-1, 0] / v[-1, 2], v[-1, 1] / v[-1, 2]
        # a line whose midpoint is a VP's image point: end points symmetric about it, in binary fractions of the offset
        hx, hy = np.float64(0.125), np.float64(0.0625)
        if midpoint_line:
            lp[1] = (vx - hx, vy - hy, vx + hx, vy + hy)
        lp[2, 2:] = lp[2, :2]                               # a zero-length segment
        lp[3] = (0.3, -0.2, 0.3 + 1e-3, -0.2 + 0.7e-3)      # far from every VP's direction: every p_lv underflows at small s
    s = np.array([SIGMAS[(i + n) % 5] for i in range(m)])
    if n >= 7:
        s[:] = np.where(s >= 1e-4, 1.2e-7, s) if (n + m) % 2 else s     # some calls without a wide sigma: line 3 hits the p_l floor
    return {"lp": lp, "cnn": sc["cnn_response"].astype(np.float32), "v": v, "s": s}


MSTEP_N = (1, 2, 3, 15, 16, 17, 63, 64, 65, 129, 511, 512, 513)
MSTEP_M = (1, 4, 5, 32, 33, 64)


def mstep_shapes():
    """Every N with two of the six M (all six M are met by N = 513 and N = 64, the two kernels' sides of N = 512)."""
    out = []
    for i, n in enumerate(MSTEP_N):
        ms = MSTEP_M if n in (64, 513) else (MSTEP_M[i % 6], MSTEP_M[(i + 3) % 6])
        out += [(n, m) for m in ms]
    return out


def bundle(rs, n, point, spread, delta):
    """n unit lines through the image point ``point`` (homogeneous (x, y, 1)) whose directions span ``spread`` radians,
    each moved off the point by noise of size delta: the weighted line matrix has s2 / s1 ~ spread and s3 / s1 ~ delta."""
    th = rs.uniform(0, np.pi) + spread * np.linspace(-0.5, 0.5, n) if n > 1 else np.array([rs.uniform(0, np.pi)])
    a, b = np.cos(th), np.sin(th)
    c = -(a * point[0] + b * point[1]) + delta * rs.uniform(-1, 1, n)
    l = np.stack([a, b, c], 1)
    return l / np.sqrt((l * l).sum(1))[:, None]


MSTEP_MAX_STDD = 1e-6
MSTEP_S_THRESH = 1e-12      # above the library's default 1e-200 so that the lower clamp can bind on representable sums


def mstep_case(n, m, hard):
    """One call of the M-step hook.  Line j belongs to VP j % M; VP k's lines are a bundle of the kind k % 12:
      0-3  noise 0, 1e-12, 1e-8, 1e-4 off the common point, directions spread over ~1 rad (s2 / s1 ~ 1)
      4-6  tight bundles: s2 / s1 ~ 1e-2, 1e-4, 1e-6 (the rows the older unit test skips)
      7    all-zero weights (hard mode: no selected line, the `continue`)      8  one NaN weight
      9    all negative weights      10  one non-zero weight (hard mode: one selected line, lapack_null_1row; its first
      coefficient is made 0 or -0.0 in two calls out of three)      11  ordinary, previous VP orthogonal to the new one
    Soft mode: VP k's weights are positive on its own lines and zero on the others (a VP with fewer than two lines of its
    own weighs all lines).  Hard mode: assoc = j % M and positive weights everywhere.
    Variance: lvsq is scaled per row so that s lands above max_stdd, between the clamps and below s_thresh; the p_vl of
    kind 5 is all zero (a NaN variance)."""
    seed = 7919 * n + 31 * m + (1 if hard else 0)
    rs = np.random.RandomState(seed)
    spreads = (1.0, 1.0, 1.0, 1.0, 1e-2, 1e-4, 1e-6)
    deltas = (0.0, 1e-12, 1e-8, 1e-4, 1e-10, 1e-10, 1e-10)
    l = np.zeros((n, 3))
    w = np.zeros((m, n))
    assoc = np.arange(n, dtype=np.int32) % m
    for k in range(m):
        kind = k % 12
        q = kind if kind <= 6 else 0
        idx = np.arange(k, n, m)
        if idx.size:
            point = rs.uniform(-0.6, 0.6, 2)
            l[idx] = bundle(rs, idx.size, point, spreads[q], deltas[q])
    for k in range(m):
        kind = k % 12
        idx = np.arange(k, n, m)
        own = np.zeros(n, dtype=bool)
        own[idx] = True
        if hard or idx.size < 2:
            w[k] = rs.uniform(0.2, 1.0, n)
        else:
            w[k, idx] = rs.uniform(0.2, 1.0, idx.size)
        if kind == 7:
            w[k] = 0.0
            if hard:
                assoc[own] = (k + 1) % m if m > 1 else -1
        elif kind == 8:
            w[k, idx[0] if idx.size else 0] = np.nan
        elif kind == 9:
            w[k] = -np.abs(w[k])
        elif kind == 10:
            if hard:
                if idx.size:
                    assoc[idx[1:]] = (k + 1) % m
                    if (n + m) % 3 != 2:                    # the reflector's sign cases: a = 0 and a = -0.0
                        b_, c_ = l[idx[0], 1], l[idx[0], 2]
                        nr = np.sqrt(b_ * b_ + c_ * c_)
                        l[idx[0]] = (0.0 if (n + m) % 3 == 0 else -0.0, b_ / nr, c_ / nr)
            else:
                w[k] = 0.0
                w[k, idx[0] if idx.size else 0] = 0.7
    levels = (1e-3, 1e-8, 1e-14, 3e-7)                      # above max_stdd | between | below s_thresh | between
    p_vl = rs.uniform(0.1, 1.0, (m, n))
    lvsq = np.zeros((m, n))
    for k in range(m):
        lvsq[k] = levels[k % 4] * rs.uniform(0.5, 1.5, n)
        if k % 12 == 5:
            p_vl[k] = 0.0
    return {"l": l, "w": w, "lvsq": lvsq, "p_vl": p_vl, "assoc": assoc if hard else None, "seed": seed}


def mstep_cur(case, ref, kind_of):
    """The previous VPs: the extended reference's new VP turned by 0.01 rad about an axis orthogonal to it (err ~ 0.01);
    kind 11 rows get a VP orthogonal to the new one (err = pi / 2 > 1.5), rows without a new VP the image centre."""
    m = len(ref)
    cur = np.zeros((m, 3))
    cur[:, 2] = 1.0
    for k, rec in enumerate(ref):
        if rec["kind"] not in ("one", "svd"):
            continue
        vp = rec["vp"].astype(np.float64)
        axis = np.cross(vp, [1.0, 0.0, 0.0] if abs(vp[0]) < 0.9 else [0.0, 1.0, 0.0])
        axis /= np.linalg.norm(axis)
        ang = np.pi / 2 if kind_of(k) == 11 else 0.01
        cur[k] = np.cos(ang) * vp + np.sin(ang) * axis
    return cur


PAIR_N = (1, 2, 3, 4, 5, 10, 11, 64, 65, 129, 130, 257, 511, 512, 513, 527, 577)


def pairwise_case(n):
    """n segments of a synthetic scene; from n = 129 on (where 1 % of the rows is at least one row), five kinds of special pairs replace the first ten segments:
    a duplicate, two crossing segments, two collinear segments that touch, two parallel ones, and a segment 1e-9 long
    beside an ordinary one."""
    sc = _scene(50000 + n, n)
    lp = sc["lp"][:n].copy()
    if n >= 129:
        rs = np.random.RandomState(n)
        c = rs.uniform(-0.5, 0.5, (5, 2))
        lp[0] = (c[0, 0], c[0, 1], c[0, 0] + 0.11, c[0, 1] + 0.07); lp[1] = lp[0]
        lp[2] = (c[1, 0] - 0.05, c[1, 1], c[1, 0] + 0.05, c[1, 1] + 0.02); lp[3] = (c[1, 0], c[1, 1] - 0.05, c[1, 0] + 0.01, c[1, 1] + 0.06)
        lp[4] = (c[2, 0], c[2, 1], c[2, 0] + 0.0625, c[2, 1] + 0.03125); lp[5] = (c[2, 0] + 0.0625, c[2, 1] + 0.03125, c[2, 0] + 0.125, c[2, 1] + 0.0625)
        lp[6] = (c[3, 0], c[3, 1], c[3, 0] + 0.08, c[3, 1] + 0.04); lp[7] = (c[3, 0] + 0.01, c[3, 1] - 0.02, c[3, 0] + 0.09, c[3, 1] + 0.02)
        lp[8] = (c[4, 0], c[4, 1], c[4, 0] + 0.8e-9, c[4, 1] + 0.6e-9); lp[9] = (c[4, 0] + 0.01, c[4, 1], c[4, 0] + 0.05, c[4, 1] + 0.03)
    return lp


INIT_CASES = [(ss, nm, kind) for ss in (500, 520, 100) for nm, kind in ((1, "few"), (5, "border"), (25, "zero_slice"), (64, "dense"))] + \
             [(500, 25, "blank"), (520, 25, "few"), (100, 64, "border")]


def init_case(ssize, num_max, kind):
    """A 20 x 20 response map of distinct float32 values and a sparse sphere image.  few: three maxima only; border:
    maxima in row / column 0 and 19 (find_maxima's index-0 quirk); zero_slice: the strongest maximum's slice of the
    sphere is all zero; dense: a random map (about 80 maxima); blank: an all-zero sphere (no VP at all)."""
    rs = np.random.RandomState(ssize * 100 + num_max)
    vals = (rs.permutation(400).astype(np.float32) + 1) / np.float32(512)       # distinct, exactly representable
    if kind == "few":
        yy, xx = np.mgrid[0:20, 0:20]
        cnn = np.zeros((20, 20))
        for cy, cx, a in ((4, 5, 1.0), (12, 14, 0.8), (17, 3, 0.6)):
            cnn += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 18.0)
        cnn = (cnn + 1e-4 * vals.reshape(20, 20) * 0).astype(np.float32)
    else:
        cnn = vals.reshape(20, 20).copy()
    if kind == "border":
        for (a, b) in ((0, 0), (0, 7), (19, 19), (8, 0), (19, 4), (5, 19), (1, 1), (1, 12)):
            cnn[a, b] = np.float32(2.0) + np.float32(a * 20 + b) / np.float32(1024)
    sphere = (rs.rand(ssize, ssize) < 0.02).astype(np.uint8) * rs.randint(1, 256, (ssize, ssize)).astype(np.uint8)
    if kind == "zero_slice":
        a, b = np.unravel_index(np.argmax(cnn), cnn.shape)
        sp = sphere[::-1, :]
        sp[a * ssize // 20:(a + 1) * ssize // 20, b * ssize // 20:(b + 1) * ssize // 20] = 0
    if kind == "blank":
        sphere[:] = 0
    return cnn, sphere


COUNT_SHAPES = [(n, m) for n in (7, 65, 257, 513) for m in (1, 5, 33)]


def counts_case(n, m):
    """A real E-step's inputs (estep_case, without the line through a VP's image point: its distance is 0 / 0) plus line
    weights with zeros in them."""
    c = estep_case(n, m, midpoint_line=False)
    rs = np.random.RandomState(n * 37 + m)
    lw = rs.uniform(0.1, 1.0, n)
    lw[::5] = 0.0
    c["lweight"] = lw
    return c


def counts_reference(pdfpar_ref, case, metric, thresh=1.96 ** 2):
    """calc_vp_line_counts on ``metric`` (M,N) with the extended lvsq: assoc, and ``clear``: the lines whose argmax
    margin (best against second best) and whose distance from the outlier threshold exceed 1e-9 relative."""
    lvsq = pdfpar_ref["lvsq"]
    s = pdfpar_ref["s"]
    mt = ld(metric)
    m_n, n = mt.shape
    assoc = np.zeros(n, dtype=np.int64)
    clear = np.ones(n, dtype=bool)
    for j in range(n):
        col = mt[:, j]
        nan = np.isnan(col)
        best = int(np.argmax(nan)) if nan.any() else int(np.argmax(col))
        if not nan.any() and m_n > 1:
            o = np.sort(col)
            if not (o[-1] - o[-2] > LD(1e-9) * abs(o[-1])):
                clear[j] = False
        thr = LD(thresh) * np.sqrt(s[best])
        dist = lvsq[j, best]
        if np.isnan(dist):
            pass                                             # NaN > thr is False: not an outlier by :504
        elif not (abs(dist - thr) > max(LD(1e-9) * thr, pdfpar_ref["b_lvsq"][j, best])):
            clear[j] = False                                 # (a distance no better known than its margin decides nothing)
        out = (dist > thr) or case["lweight"][j] == 0
        assoc[j] = -1 if out else best
    return assoc, clear


# =============================================================================================================
# the bars, applied to one backend's outputs (the HIP kernels, the host build of the device source, or the oracle).
# Each check returns the worst ratio error / bar it saw (<= 1 when it passes); WORST keeps the maximum per phase.
# =============================================================================================================
WORST = {}


def _note(phase, ratio):
    ratio = float(ratio)
    WORST[phase] = max(WORST.get(phase, 0.0), ratio)
    return ratio


def _ratio(err, bound):
    """max of err / bound over the elements with a finite bound (a zero error never fails a zero bound)."""
    err = np.atleast_1d(np.asarray(err, dtype=LD))
    bound = np.atleast_1d(np.asarray(bound, dtype=LD))
    err, bound = np.broadcast_arrays(err, bound)
    ok = np.isfinite(bound) & np.isfinite(err)
    if not ok.any():
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err[ok] == 0, LD(0), err[ok] / bound[ok])
    return float(r.max())


def same_pattern(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b))


def ordinary_vps(v):
    """VPs for which the project's flat bars are meant: away from the plane z = 0 and from asin's poles."""
    v = np.asarray(v)
    return (np.abs(v[:, 2]) > 1e-2) & (np.abs(v[:, 1]) < 0.99)


def check_estep(out, case, ref, orc):
    """out: dict p_v (M), lvsq (N,M), p_vl (M,N), p_l (N) or None, s (M).  orc: the float64 oracle's PDF."""
    assert np.array_equal(out["s"], np.maximum(case["s"], 1e-200)), "s is floored in place at 1e-200"
    pairs = [("p_v", orc.v), ("lvsq", orc.lvsq), ("p_vl", orc.vl)] + ([("p_l", orc.l)] if out.get("p_l") is not None else [])
    for key, want in pairs:
        assert same_pattern(out[key], want), "NaN / Inf pattern of %s differs from the float64 oracle's" % key
    ordv = ordinary_vps(case["v"])
    fin = np.isfinite(np.asarray(orc.v))
    e = np.abs(ld(out["p_v"]) - ref["p_v"])
    r = [_ratio(e[fin], ref["b_pv"][fin])]
    sel = fin & ordv
    r.append(_ratio(e[sel], 1e-11 * np.abs(ref["p_v"][sel])))                       # flat: p_v 1e-11 relative
    fin = np.isfinite(np.asarray(orc.lvsq))
    e = np.abs(ld(out["lvsq"]) - ref["lvsq"])
    r.append(_ratio(e[fin], ref["b_lvsq"][fin]))
    well = fin & ordv[None, :] & (ref["b_lvsq"] <= LD(1e-13))                        # flat: lvsq 1e-13, where the chain is well conditioned
    r.append(_ratio(e[well], LD(1e-13)))
    fin = np.isfinite(np.asarray(orc.vl))
    e = np.abs(ld(out["p_vl"]) - ref["p_vl"])
    r.append(_ratio(e[fin], ref["b_pvl"][fin]))
    if out.get("p_l") is not None:
        fin = np.isfinite(np.asarray(orc.l))
        e = np.abs(ld(out["p_l"]) - ref["p_l"])
        r.append(_ratio(e[fin], ref["b_pl"][fin]))
    names = ("p_v", "p_v flat", "lvsq", "lvsq flat", "p_vl", "p_l")
    for nm, x in zip(names, r):
        _note("estep " + nm, x)
        assert x <= 1.0, "E-step %s: error / bar = %.3g" % (nm, x)
    return max(r)


def lapack_one_row(row):
    """V[:, 2] of numpy.linalg.svd on one row (full_matrices, as calc_new_vanishing_point calls it for fewer than three
    rows), normalised, signed by z."""
    _, _, vt = np.linalg.svd(np.asarray(row, dtype=np.float64)[None, :], full_matrices=True)
    vp = vt[2] / np.linalg.norm(vt[2])
    return vp * np.sign(vp[2])


def check_mstep(out, case, ref, cur, hard, max_stdd=MSTEP_MAX_STDD, s_thresh=MSTEP_S_THRESH):
    vp, s, err, removed = out
    worst = 0.0
    l = case["l"]
    for k, rec in enumerate(ref):
        tag = "VP %d (kind %d)" % (k, k % 12)
        if rec["kind"] in ("skip", "none"):
            assert removed[k] == (0 if rec["kind"] == "skip" else 1), tag
            assert err[k] == -1.0 and np.all(vp[k] == 0) and s[k] == -1.0, tag + ": nothing may be written"
            continue
        # the bar without a condition number, |diag(r) l vp| <= s3 + c(N) u s1, as (residual - s3) / (c(N) u s1) <= 1
        r = [_ratio(max(residual(l, rec["r"], vp[k]) - rec["sv"][2], LD(0)), rec["res_bound"] - rec["sv"][2])]
        d_vp = LD(np.inf)
        s1, s2, s3 = rec["sv"]
        if rec["kind"] == "one":
            # one row: the vector is LAPACK's choice in a two-dimensional null space.  Ten rounded operations on numbers
            # of size <= 2 in the reflector, and as many in LAPACK's: 1e-14 (90 u) holds both
            want = lapack_one_row(l[np.nonzero(rec["sel"])[0][0]])
            assert abs(np.sqrt(float((ld(vp[k]) ** 2).sum())) - 1) <= 8 * float(U), tag + ": not a unit vector"
            d_vp = LD(1e-14)
            r.append(_ratio(np.abs(vp[k] - want).max(), d_vp))
        elif s2 > c_of_n(l.shape[0]) * U * s1 * 4:                                   # rank >= 2: the vector is determined
            assert abs(np.sqrt(float((ld(vp[k]) ** 2).sum())) - 1) <= 8 * float(U), tag + ": not a unit vector"
            d_vp = rec["vec_bound"]
            e = np.sqrt(((ld(vp[k]) - rec["vp"]) ** 2).sum())
            r.append(_ratio(e, d_vp))
            if s2 >= LD(1e-3) * s1 and s3 <= LD(1e-2) * s2:
                r.append(_ratio(e, LD(1e-9)))                                        # flat: M-step VP 1e-9
        # variance
        if np.isnan(rec["s"]):
            assert np.isnan(s[k]) and removed[k] == 1 and err[k] == -1.0, tag + ": a NaN variance removes the VP"
        else:
            raw = rec["s_raw"]
            lo_clamp = (not hard) and raw < LD(s_thresh) * (1 - rec["rel_s"])
            hi_clamp = raw > LD(max_stdd) * (1 + rec["rel_s"])
            if hi_clamp:
                assert s[k] == max_stdd, tag + ": the upper clamp binds exactly"
            elif lo_clamp:
                assert s[k] == s_thresh, tag + ": the lower clamp binds exactly"
            else:
                r.append(_ratio(abs(LD(s[k]) - rec["s"]), rec["rel_s"] * rec["s"]))
            if hard and raw < LD(s_thresh) * (1 - rec["rel_s"]):
                assert removed[k] == 1 and err[k] == -1.0, tag + ": s < s_thresh removes the VP in hard mode"
            elif np.isfinite(d_vp):
                want = rec["vp"] if rec["kind"] == "svd" else ld(lapack_one_row(l[np.nonzero(rec["sel"])[0][0]]))
                e_ref, b_err = err_reference(cur[k], want, d_vp)
                r.append(_ratio(abs(LD(err[k]) - e_ref), b_err))
                if abs(e_ref - LD(1.5)) > b_err:
                    assert removed[k] == int(e_ref > LD(1.5)), tag + ": err > 1.5 decides the removal"
        for x in r:
            assert x <= 1.0, "%s: error / bar = %.3g in %s" % (tag, x, ["%.3g" % y for y in r])
        worst = max(worst, max(r))
    _note("mstep", worst)
    return worst


def check_pairwise(out, lp, ref, orc):
    """out: lsim, lscore, langle.  orc: the oracle's three (calc_lsim sigma = 1, line_rating_knn k2 = 4, lines_angles)."""
    lsim, lscore, langle = out
    n = lp.shape[0]
    for got, want, nm in zip(out, orc, ("lsim", "lscore", "langle")):
        assert same_pattern(got, want), "NaN / Inf pattern of %s differs from the float64 oracle's" % nm
    assert np.array_equal(lsim, lsim.T, equal_nan=True)
    clear = ref["clear"]
    assert (~clear).sum() <= n // 100, "more than 1 %% of the rows are left out of the score comparison: %d of %d" % ((~clear).sum(), n)
    r = []
    fin = np.isfinite(orc[0])
    r.append(_ratio(np.abs(lsim - orc[0])[fin], LD(1e-12)))                          # flat bars, against NumPy ...
    r.append(_ratio(np.abs(ld(lsim) - ref["lsim"])[fin], LD(1e-12)))                 # ... and against the extended reference
    fin = np.isfinite(orc[1]) & clear
    r.append(_ratio(np.abs(lscore - orc[1])[fin], LD(1e-12)))
    r.append(_ratio(np.abs(ld(lscore) - ref["lscore"])[fin], LD(1e-12)))
    fin = np.isfinite(orc[2])
    r.append(_ratio(np.abs(langle - orc[2])[fin], LD(1e-13)))
    r.append(_ratio(np.abs(ld(langle) - ref["langle"])[fin], np.maximum(ref["b_langle"][fin], 0)))
    for nm, x in zip(("lsim", "lsim ext", "lscore", "lscore ext", "langle", "langle ext"), r):
        _note("pairwise " + nm, x)
        assert x <= 1.0, "pairwise %s (N = %d): error / bar = %.3g" % (nm, n, x)
    return max(r)


def check_counts(out, case, assoc_ref, clear):
    counts, counts_w, assoc = out
    n = assoc_ref.shape[0]
    assert (~clear).sum() <= n // 100, "more than 1 %% of the lines are left out: %d of %d" % ((~clear).sum(), n)
    assert np.array_equal(assoc[clear], assoc_ref[clear])
    if clear.all():
        m = counts.shape[0]
        assert np.array_equal(counts, np.bincount(assoc_ref[assoc_ref >= 0], minlength=m).astype(np.float64))
    m = counts.shape[0]
    assert np.array_equal(counts, np.bincount(assoc[assoc >= 0], minlength=m).astype(np.float64))      # consistent with its own assoc
    cw = np.array([case["lweight"][assoc == k].sum() for k in range(m)])
    assert np.abs(counts_w - cw).max() <= n * float(U) * max(cw.max(), 1.0) * 2
