"""VP set maintenance under the reference's other two distance measures, "dotprod" and "area": extended-precision
restatements of the two distances, of calc_vp_line_counts and of merge_vps per measure, the margins of every decision they
take, and the seeded case generators shared by scripts/make_vpset_measure_goldens.py, tests/test_vp_set_measures.py (CPU)
and tests/test_gpu_vp_set_measures.py (the HIP kernels).  CPU only.  The "angle" forms, the margins' vocabulary and the
geometry of the cases are tests/vp_set_reference.py's, imported and left as they are.

Restated from the reference's source in ``np.longdouble`` (not from the device code):

  dotprod  counts: |vp[m] . l[n]| (vp_localisation.py:496); merge: calc_lvsq_dotprod (probability_functions.py:150-154)
  area     counts: calc_lvsq_area_single (probability_functions.py:227-249); merge: calc_lvsq_area (:179-209)
  counts   vp_localisation.py:482-512 with its branch on the measure (:495-500); every operand as the caller gives it
  merge    vp_localisation.py:633-684, its measure handed to calc_probabilities (:658): vp_set_reference.merge_reference
           with estep_reference.reference(measure, ...) in the place of the "angle" E-step

Bars.  The distances carry estep_reference's bounds for their measure (dotprod: 3 u sum |l_i v_i| on the dot product;
area: the interval bound of lvsq_area, infinite below a relative radicand of 1e-12 -- such a pair has no clear margin and
no committed case holds one).  Against the restatements a merge is held to vp_set_reference's bars widened by those
bounds.  Against the reference's recorded results: directions 1e-4 rad and variances GOLDEN_S_FACTOR * GOLDEN_S_REL[measure]
relative, where GOLDEN_S_REL is the largest relative deviation of the reference's recorded s from the restatement over
the committed cases of that measure, measured on the CPU by tests/test_vp_set_measures.py::test_golden_variance_bar and
rounded up:

  dotprod  measured 6.32e-16 -> 6.4e-16
  area     measured 7.74e-15 -> 7.8e-15

The factor 4 (vp_set_reference.GOLDEN_S_FACTOR) allows for the device's other summation order.  Neither number was fitted
to device output.
"""
import os

import numpy as np

import estep_reference as ER
import vp_set_reference as R
from em_phase_reference import LD, U, ld, null_vector_reference, residual, c_of_n, _ratio
from vp_set_reference import Margins, MARGIN_MIN, GOLDEN_S_FACTOR, PARITY_RAD, _rel, _argmax_first, _argmax_margin  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "vpset_measures")
MEASURES = ("dotprod", "area")                  # the new ones; "angle" stays with vp_set_reference
GOLDEN_S_REL = {"dotprod": 6.4e-16, "area": 7.8e-15}


# =============================================================================================================
# the distance of the outlier test
# =============================================================================================================
def dist_single(measure, v, lp, l):
    """(dist, bound) of one (VP, line) pair as calc_vp_line_counts evaluates it (:495-500).  NaN where the reference's is."""
    if measure == "angle":
        return R.lvsq_single(v, lp)
    if measure == "dotprod":
        terms = ld(v) * ld(l)
        return abs(terms.sum()), 3 * U * np.abs(terms).sum()
    lvsq, bound, _ = ER.lvsq_area(np.asarray(v, dtype=np.float64)[None, :], np.asarray(lp, dtype=np.float64)[None, :])
    return lvsq[0, 0], bound[0, 0]


def counts_reference(measure, vp, lp, l, s, metric, lweights, thresh=2.57, vp_assoc=None):
    """(counts, counts_weighted (longdouble, the reference's running sum :509-510), vp_assoc, margins, inside) -- inside:
    per associated line, whether :504 was false (None for a line that was skipped)."""
    vp = np.asarray(vp, dtype=np.float64)
    n_l, m_n = lp.shape[0], vp.shape[0]
    mg = Margins()
    if vp_assoc is None:
        mt = ld(metric)
        assoc = np.array([_argmax_first(mt[:, j]) for j in range(n_l)], dtype=np.int64)
        _argmax_margin(mg, mt)
    else:
        assoc = np.array(vp_assoc, dtype=np.int64)
    counts = np.zeros(m_n)
    cw = np.zeros(m_n, dtype=LD)
    inside = [None] * n_l
    for n in range(n_l):
        m = assoc[n]
        if m > -1:
            dist, b = dist_single(measure, vp[m], lp[n], None if l is None else l[n])
            with np.errstate(invalid="ignore"):
                thr = LD(thresh) * np.sqrt(ld(s[m]))
            out = False
            if not (np.isnan(dist) or np.isnan(thr)):           # a NaN makes :504 false: the line counts
                mg.note("outlier", _rel(dist, thr, b + 4 * U * thr) if np.isfinite(b) else LD(0))
                out = bool(dist > thr)
            inside[n] = not out
            if out or lweights[n] == 0:
                assoc[n] = -1
            else:
                counts[m] += 1
                cw[m] += LD(lweights[n])
    return counts, cw, assoc, mg, inside


# A NaN distance under "area".  In exact arithmetic b <= c (the first end point is c away from the midpoint, through which
# the line of :240 passes), with equality where the VP's direction is at right angles to the segment; the radicand of :245
# is negative only through rounding.  area_radicand_fp64 is that radicand as IEEE double evaluates the chain of
# calc_lvsq_area_single -- products and sums rounded one by one, np.dot / np.linalg.norm of two components as one fused step
# (em_ctx.hpp's note on NumPy's BLAS) -- and serves to pick inputs whose fp64 radicand IS negative; what is asserted of
# them needs no such care: a NaN distance and a distance of nearly 0 both leave :504 false, and the line counts.
def _fma(a, b, c):
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def area_radicand_fp64(v, q):
    v, q = np.asarray(v, dtype=np.float64), np.asarray(q, dtype=np.float64)
    norm2 = lambda x, y: np.sqrt(np.float64(_fma(y, y, x * x)))
    vx, vy = v[0] / v[2], v[1] / v[2]
    mx, my = 0.5 * (q[0] + q[2]), 0.5 * (q[1] + q[3])
    nrm = norm2(vy, -vx)
    b = abs(((vy / nrm) * q[0] + (-vx / nrm) * q[1]) + (vx * my - vy * mx) / nrm)
    c = norm2(mx - q[2], my - q[3])
    return c * c - b * b


def negative_radicand_case(n=65, seed=11):
    """One VP and n segments at right angles to its direction as seen from their midpoints (to within rounding), at least
    one of which has a negative fp64 radicand: (vp (1, 3), lp (n, 4))."""
    rs = np.random.RandomState(seed)
    pt = rs.uniform(-0.5, 0.5, 2)
    vp = R._unit([[pt[0], pt[1], 1.0]])
    vx, vy = vp[0, 0] / vp[0, 2], vp[0, 1] / vp[0, 2]
    nr = np.hypot(vx, vy)
    mid = rs.uniform(-1, 1, (n, 2))
    half = rs.uniform(0.05, 0.2, n)[:, None] * (np.array([-vy, vx]) / nr)[None, :]
    lp = np.c_[mid - half, mid + half]
    assert any(area_radicand_fp64(vp[0], q) < 0 for q in lp)
    return vp, lp


# =============================================================================================================
# merge
# =============================================================================================================
def merge_reference(measure, vi, s, l, thresh, lw, lsim, wbias, pdfpar, lp, max_stdd=0.01):
    """vp_set_reference.merge_reference under ``measure``: the same loop, records and margins; the E-step of every round
    (:658) is estep_reference.reference(measure, ...), whose bounds widen s_k's and the row weights'."""
    if measure == "angle":
        return R.merge_reference(vi, s, l, thresh, lw, lsim, wbias, pdfpar, lp, max_stdd)
    v = ld(np.asarray(vi, dtype=np.float64)).copy()
    s = ld(s).copy()
    kept = list(range(v.shape[0]))
    mg = Margins()
    rounds = []
    n_l = lp.shape[0]
    while v.shape[0] > 1:
        ang = R.angle_matrix(v)
        m_n = v.shape[0]
        flat = ang.ravel()
        p = int(np.argmin(flat))
        j, k = p // m_n, p % m_n
        others = np.delete(flat, [j * m_n + k, k * m_n + j])
        if others.size:
            mg.note("min-angle argmin", _rel(others.min(), flat[p], 8 * U))
        mg.note("min_angle < thresh", _rel(flat[p], LD(thresh), 8 * U))
        if not flat[p] < thresh:
            break
        e = ER.reference(measure, v.astype(np.float64), l, lp, s.astype(np.float64), pdfpar=pdfpar)
        s = e["s"].copy()                                        # calc_plv floors s in place (:139)
        w, b_w = R.weight_matrix_reference(e["p_vl"], e["b_p_vl"], lw, lsim, wbias)
        r = w[j] + w[k]
        rec = {"j": j, "k": k, "none": bool(n_l == 0 or r.max() == 0)}
        pq = e["p_vl"][k] + e["p_vl"][j]
        lq = LD(0.5) * (e["lvsq"][:, j] + e["lvsq"][:, k])
        sv, sp = (lq * pq).sum(), pq.sum()
        d_sv = (LD(0.5) * (e["b_lvsq"][:, j] + e["b_lvsq"][:, k]) * pq + lq * (e["b_p_vl"][k] + e["b_p_vl"][j])).sum()
        d_sp = (e["b_p_vl"][k] + e["b_p_vl"][j]).sum()
        s_k = sv / sp
        rec["s_k"] = s_k
        rec["rel_s"] = (2 * n_l + 8) * U + 2 * U * (abs(np.log(sv)) + abs(np.log(sp))) + d_sv / sv + d_sp / sp
        s[k] = s_k                                               # :666, before the abort test
        mg.note("s[k] > max_stdd", _rel(s_k, LD(max_stdd), rec["rel_s"] * s_k) if np.isfinite(rec["rel_s"]) else LD(0))
        if not rec["none"]:
            rmax = r.max()
            nv = null_vector_reference(l, (r / rmax).astype(np.float64))
            rec.update(nv)
            rec["r"] = (r / rmax).astype(np.float64)
            b_r = (b_w[j] + b_w[k]) / rmax + 4 * U * r / rmax
            rec["b_r"] = np.sqrt((b_r * b_r).sum())              # |delta(diag(r) l) x| <= |delta r|_2 for unit rows, unit x
        rec["ok"] = (not rec["none"]) and not (s_k > max_stdd)
        rounds.append(rec)
        if not rec["ok"]:
            break
        v[k] = rec["vp"]
        v = np.delete(v, j, axis=0)
        s = np.delete(s, j)
        del kept[j]
    return {"v": v, "s": s, "kept": np.array(kept, dtype=np.int64), "rounds": rounds, "margins": mg}


# =============================================================================================================
# case generators (seeded; inputs only)
# =============================================================================================================
COUNT_N, COUNT_M = R.COUNT_N, R.COUNT_M
# The variances of the counts cases, by M.  "area" distances are lvsq-like and meet thresh sqrt(s) at vp_set_reference's
# own s (4e-12).  |vp . l| finds no inlier there: at 1e8 times that s the M = 2 cases (one VP at infinity, whose lines are
# far from it) have 28 % to 50 % of their associated lines inside the threshold, but with every line on its nearest VP --
# M = 1, and M = 64 under the argmax of the metric -- 90 % to 98 % are inside; those shapes take 1e7 times (33 % to 72 %).
S_SCALE = {"dotprod": {1: 4e-5, 2: 4e-4, 64: 4e-5}, "area": {1: 4e-12, 2: 4e-12, 64: 4e-12}}
INSIDE_MIN, INSIDE_MAX, INSIDE_FROM_N = 0.1, 0.9, 63


def inside_fraction(inside):
    seen = [x for x in inside if x is not None]
    return sum(seen) / float(len(seen)) if seen else 0.0


def counts_cases(measure):
    """name -> inputs: vp_set_reference.counts_cases' geometry, seeds and alternations (thresh between 2.57 and 1.96^2;
    every other case a vp_assoc with -1 entries; every fifth line of weight zero; one VP of the M = 2 cases with
    v[2] == 0), with the lines ``l`` and the measure's own s.  A seed is taken if every margin is clear and, from N = 63
    on, between 10 % and 90 % of the associated lines lie inside the threshold: both branches of :504 are exercised."""
    out = {}
    q = 0
    for n in COUNT_N:
        for m in COUNT_M:
            for seed in range(1000):
                rs = np.random.RandomState(7919 * n + 104729 * m + seed)
                vp, pts = R._vps_in_image(rs, m)
                own = rs.randint(0, m, n)
                lp = np.concatenate([R._segments_to(rs, pts[own[i]], 1, 0.12) for i in range(n)])
                if m == 2:
                    vp[1] = R._unit([0.6, 0.8, 0.0])
                s = rs.uniform(0.5, 2.0, m) * S_SCALE[measure][m]
                dist = np.array([[float(R.lvsq_single(vp[k], lp[i])[0]) for i in range(n)] for k in range(m)])
                metric = 1.0 / (1e-6 + np.nan_to_num(dist, nan=1.0)) * rs.uniform(0.8, 1.2, (m, n))
                lw = rs.uniform(0.1, 1.0, n)
                lw[::5] = 0.0
                thresh = 2.57 if q % 2 == 0 else 1.96 ** 2
                assoc = None
                if q % 2 == 1:
                    assoc = own.astype(np.int64)
                    assoc[::4] = -1
                case = {"vp": vp, "lp": lp, "l": R._lines_of(lp), "s": s, "metric": metric, "lweights": lw,
                        "thresh": np.float64(thresh)}
                if assoc is not None:
                    case["vp_assoc"] = assoc
                ref = counts_reference(measure, vp, lp, case["l"], s, metric, lw, thresh, assoc)
                if ref[3].clear() and (n < INSIDE_FROM_N or INSIDE_MIN <= inside_fraction(ref[4]) <= INSIDE_MAX):
                    break
            else:
                raise AssertionError("no clear %s counts case for N = %d, M = %d" % (measure, n, m))
            out["counts_n%d_m%d" % (n, m)] = case
            q += 1
    return out


# What the reference does with vp_set_reference.MERGE_SPECS' layouts under each measure: (max_stdd, merges carried out,
# what ends the loop).  At 0.01 it merges under all three; "dotprod" gives up at 1e-3 already, the EM's own bound under
# that measure (:200), because the merged s[k] is 1e-3 to 2e-3; of the chain of three close VPs "area" merges one pair.
MERGE_OUTCOMES = {
    "dotprod": {
        "merge_m1": (0.01, 0, "one VP"), "merge_m2_below": (0.01, 1, "one VP"), "merge_m2_above": (0.01, 0, "angle"),
        "merge_chain3": (0.01, 2, "angle"), "merge_abort": (1e-3, 0, "max_stdd"), "merge_zero_weights": (0.01, 0, "none"),
        "merge_n1": (0.01, 1, "angle"), "merge_n64": (0.01, 1, "angle"), "merge_n65": (0.01, 1, "angle"),
    },
    "area": {
        "merge_m1": (0.01, 0, "one VP"), "merge_m2_below": (0.01, 1, "one VP"), "merge_m2_above": (0.01, 0, "angle"),
        "merge_chain3": (0.01, 1, "angle"), "merge_abort": (1e-6, 0, "max_stdd"), "merge_zero_weights": (0.01, 0, "none"),
        "merge_n1": (0.01, 1, "angle"), "merge_n64": (0.01, 1, "angle"), "merge_n65": (0.01, 1, "angle"),
    },
}


def merge_case(measure, name, attempt=0):
    """vp_set_reference.merge_case with the measure's max_stdd (inputs without lsim and the prior, which the recorder adds)."""
    c = R.merge_case(name, attempt)
    c["max_stdd"] = np.float64(MERGE_OUTCOMES[measure][name][0])
    return c


# =============================================================================================================
# the committed cases
# =============================================================================================================
def golden_names(measure, prefix):
    head = measure + "_" + prefix
    return sorted(f[len(measure) + 1:-4] for f in os.listdir(GOLDEN) if f.startswith(head) and f.endswith(".npz"))


def golden(measure, name):
    with np.load(os.path.join(GOLDEN, "%s_%s.npz" % (measure, name))) as z:
        return {k: z[k] for k in z.files}


def pdfpar_of(g):
    return (R._grid(), g["prior_weights"], float(g["prior_sigma"]))


def merge_reference_of(measure, g):
    return merge_reference(measure, g["v"], g["s"], g["l"], float(g["thresh"]), g["lw"], g["lsim"], float(g["wbias"]),
                           pdfpar_of(g), g["lp"], float(g["max_stdd"]))


# =============================================================================================================
# the bars, as the CPU twin and the GPU tests apply them to one result
# =============================================================================================================
COUNTS = ["counts_n%d_m%d" % (n, m) for n in COUNT_N for m in COUNT_M]


def counts_ref(measure, g):
    return counts_reference(measure, g["vp"], g["lp"], g["l"], g["s"], g["metric"], g["lweights"], float(g["thresh"]),
                               g.get("vp_assoc"))


def angle_between(a, b):
    a, b = ld(a), ld(b)
    c = abs(np.dot(a, b)) / np.sqrt(np.dot(a, a) * np.dot(b, b))
    return float(np.arccos(min(c, LD(1))))


def check_null_vector(rec, l, r, vp, widen=LD(0)):
    """the bars em_phase_reference.check_mstep applies to the same device function"""
    s1, s2, s3 = rec["sv"]
    assert _ratio(max(residual(l, r, vp) - s3, LD(0)), rec["res_bound"] - s3 + widen) <= 1.0, "null-vector residual"
    if s2 > c_of_n(l.shape[0]) * U * s1 * 4:
        assert abs(np.sqrt(float((ld(vp) ** 2).sum())) - 1) <= 8 * float(U)
        e = np.sqrt(((ld(vp) - rec["vp"]) ** 2).sum())
        assert _ratio(e, rec["vec_bound"] + widen / (s2 - s3)) <= 1.0, "null vector"


def check_counts(got, measure, g):
    counts, cw, assoc = got
    assert np.array_equal(counts, g["out_counts"]) and np.array_equal(assoc, g["out_vp_assoc"]) and assoc.dtype == np.int64
    ref_cw = counts_ref(measure, g)[1]
    assert np.all(np.abs(ld(cw) - ref_cw) <= g["lp"].shape[0] * U * ref_cw)


def check_merge(got, measure, g, ref):
    v, s, kept, flags = got
    s_bar = GOLDEN_S_FACTOR * GOLDEN_S_REL[measure]
    assert np.array_equal(kept, g["out_kept"]) and v.shape == g["out_v"].shape and flags == 0
    rounds = ref["rounds"]
    rank1 = any((not q["none"]) and q["sv"][1] <= 1e-6 * q["sv"][0] for q in rounds)
    for k in range(v.shape[0]):
        if not rank1:
            assert angle_between(v[k], g["out_v"][k]) <= PARITY_RAD
    rel = np.abs(ld(s) - ld(g["out_s"])) / np.abs(ld(g["out_s"]))
    print("s against the golden, error / bar:", float(rel.max() / s_bar))
    assert np.all(rel <= s_bar)
    if len(rounds) == 1:     # (later rounds start from the device's own VPs: first-order bars hold for the first)
        q = rounds[0]
        k_out = int(np.nonzero(kept == g["out_kept"][q["k"] - (1 if q["ok"] and q["j"] < q["k"] else 0)])[0][0]) if q["ok"] else q["k"]
        assert abs(LD(s[k_out]) - q["s_k"]) <= q["rel_s"] * q["s_k"], "variance of the merged VP"
        if q["ok"]:
            check_null_vector(q, g["l"], q["r"], v[k_out], widen=q["b_r"])
        else:
            assert s[k_out] != g["s"][k_out] and np.array_equal(v, g["v"]), "a merge given up returns the changed s[k] (:666-668)"
