"""Extended-precision restatements of the reference's VP set maintenance, the margins of every decision they take, and
the seeded case generators shared by scripts/make_vpset_goldens.py, tests/test_vp_set.py (CPU) and
tests/test_gpu_vp_set.py (the HIP kernels).  CPU only.

Restated from the reference's source in ``np.longdouble`` (not from the device code):

  counts   vp_localisation.py:482-512 (calc_vp_line_counts) with probability_functions.py:212-224 (calc_lvsq_single)
  split    vp_localisation.py:527-630 (split_best_vp) with :715-724 (lines_points_cosangle, f = 2) and scikit-learn's
           AgglomerativeClustering(linkage='average', connectivity=D, metric='precomputed', n_clusters=2)
  merge    vp_localisation.py:633-697 (merge_vps, calc_angle_to_other_vp) with calc_probabilities, weight_matrix (:515-524)
           and calc_new_vanishing_point (:453-479)

Every decision notes its MARGIN: the relative distance of the two sides of the comparison, less what rounding can move
them.  A case belongs to the goldens only if every margin exceeds MARGIN_MIN; the generators below produce only such
cases and tests/test_vp_set.py verifies it over the committed files with no case left out.

Bars.  Against these restatements: the null-vector residual and vector bounds of em_phase_reference
(null_vector_reference) and the variance bound of its check_mstep, (2 N + 8) u + 2 u (|ln sv| + |ln sp|), each widened
by the first-order propagation of the E-step's own bounds (estep_reference's b_lvsq, b_pvl) through the non-negative
sums in front of them.  Against the reference's recorded results (LAPACK SVD): directions 1e-4 rad (the project's
parity bar) and variances GOLDEN_S_FACTOR * GOLDEN_S_REL relative, where GOLDEN_S_REL = 8.2e-14 is the largest relative
deviation of the reference's recorded s from the restatement over all committed cases, measured on the CPU by
tests/test_vp_set.py::test_golden_variance_bar (8.17e-14, rounded up), and the factor 4 allows for the device's
other summation order.  Neither number was fitted to device output.
"""
import numpy as np

from em_phase_reference import LD, U, PI, ld, null_vector_reference, residual, estep_reference, _ratio  # noqa: F401
from em_smoother_reference import smooth_reference

MARGIN_MIN = LD(1e-9)
GOLDEN_S_REL = 8.2e-14
GOLDEN_S_FACTOR = 4
PARITY_RAD = 1e-4            # README: the project's parity bar for VP directions
PI64 = LD(np.pi)             # the reference's `pi` is the fp64 constant


class Margins(dict):
    """name -> smallest margin seen."""

    def note(self, name, value):
        value = LD(value)
        if name not in self or value < self[name]:
            self[name] = value

    def clear(self):
        return all(v > MARGIN_MIN for v in self.values())

    def worst(self):
        return min(self.items(), key=lambda kv: kv[1]) if self else ("none", LD(np.inf))


def _rel(a, b, slack=0):
    """relative distance of a and b, less an absolute slack"""
    scale = max(abs(a), abs(b))
    if scale == 0:
        return LD(0)
    return (abs(a - b) - slack) / scale


def _argmax_first(col):
    """np.argmax of a column: first maximum, a NaN counts as the maximum."""
    nan = np.isnan(col)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(col))


def _argmax_margin(mg, mt):
    for j in range(mt.shape[1]):
        col = mt[:, j]
        if mt.shape[0] > 1 and not np.isnan(col).any():
            o = np.sort(col)
            mg.note("argmax", _rel(o[-1], o[-2]))


# =============================================================================================================
# counts
# =============================================================================================================
def lvsq_single(v, q):
    """calc_lvsq_single and the rounding bound of its fp64 evaluation (em_phase_reference.estep_reference's b_lvsq)."""
    v, q = ld(v), ld(q)
    with np.errstate(divide="ignore", invalid="ignore"):
        vx, vy = v[0] / v[2], v[1] / v[2]
        lmx, lmy = LD(0.5) * (q[0] + q[2]), LD(0.5) * (q[1] + q[3])
        v1x, v1y, v2x, v2y = lmx - vx, lmy - vy, q[0] - q[2], q[1] - q[3]
        n1 = np.sqrt(v1x * v1x + v1y * v1y)
        cc = 1 - abs((v1x * v2x + v1y * v2y) / (n1 * np.sqrt(v2x * v2x + v2y * v2y)))
        d_cc = U * (15 + (abs(vx) + abs(vy) + abs(lmx) + abs(lmy)) / n1)
    return cc * cc, 2 * abs(cc) * d_cc + d_cc * d_cc + U * cc * cc


def counts_reference(vp, lp, s, metric, lweights, thresh=2.57, vp_assoc=None):
    """(counts, counts_weighted (longdouble, the reference's running sum :509-510), vp_assoc, margins)."""
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
    for n in range(n_l):
        m = assoc[n]
        if m > -1:
            dist, b = lvsq_single(vp[m], lp[n])
            with np.errstate(invalid="ignore"):
                thr = LD(thresh) * np.sqrt(ld(s[m]))
            out = False
            if not (np.isnan(dist) or np.isnan(thr)):           # a NaN makes :504 false: the line counts
                mg.note("outlier", _rel(dist, thr, b + 4 * U * thr))
                out = dist > thr
            if out or lweights[n] == 0:
                assoc[n] = -1
            else:
                counts[m] += 1
                cw[m] += LD(lweights[n])
    return counts, cw, assoc, mg


# =============================================================================================================
# split
# =============================================================================================================
def ldist_matrix(lp):
    """Ldist (:568-572): 1 - cos(clip(2 acos |cos|, -pi/2, pi/2))."""
    q = ld(lp)
    vx, vy = q[:, 0] - q[:, 2], q[:, 1] - q[:, 3]
    nr = np.sqrt(vx * vx + vy * vy)
    c = np.abs((vx[:, None] * vx[None, :] + vy[:, None] * vy[None, :]) / (nr[:, None] * nr[None, :]))
    dphi = np.abs(np.arccos(np.clip(c, -1, 1)))
    d = 1 - np.cos(np.clip(2 * dphi, -PI64 / 2, PI64 / 2))
    np.fill_diagonal(d, 0)
    return d


def cluster2_reference(d, mg):
    """Average-linkage agglomeration over the graph of d's non-zero entries, as scikit-learn's linkage_tree builds it: the
    closest connected pair merges; a neighbour of both gets the size-weighted mean, a neighbour of one keeps its distance;
    the tree is cut at the root and the child with the larger node id -- the cluster formed last -- is label 0.  Returns
    labels, or None where the graph falls apart (scikit-learn then completes it: not restated)."""
    n = d.shape[0]
    dist = {}
    for a in range(n):
        for b in range(a):
            if d[a, b] + d[b, a] != 0:
                dist[(b, a)] = d[a, b]
    members = {a: [a] for a in range(n)}
    node = n
    while len(members) > 2:
        if not dist:
            return None
        order = sorted(dist.items(), key=lambda kv: kv[1])
        (a, b), best = order[0]
        if len(order) > 1:
            mg.note("closest pair", _rel(order[1][1], best))
        na, nb = len(members[a]), len(members[b])
        new = {}
        for c in members:
            if c in (a, b):
                continue
            da = dist.pop((min(a, c), max(a, c)), None)
            db = dist.pop((min(b, c), max(b, c)), None)
            if da is not None and db is not None:
                new[c] = (na * da + nb * db) / LD(na + nb)
            elif da is not None or db is not None:
                new[c] = da if da is not None else db
        del dist[(a, b)]
        members[node] = members.pop(a) + members.pop(b)
        for c, val in new.items():
            dist[(c, node)] = val
        node += 1
    labels = np.zeros(n, dtype=np.int64)
    first, second = sorted(members, reverse=True)
    labels[members[second]] = 1
    return labels


def split_reference(vi, s, lp, l, w, lw, langle, min_diff=1e-4):
    """split_best_vp on one slice: dict of v (M', 3), s, split (index or -1), labels (N, -1 outside the worst VP's set;
    None where no VP qualified), the null-vector records of the clusters and the margins."""
    vi = np.asarray(vi, dtype=np.float64)
    m_n, n_l = vi.shape[0], lp.shape[0]
    mg = Margins()
    wl = ld(w)
    assoc = np.array([_argmax_first(wl[:, j]) for j in range(n_l)], dtype=np.int64)
    _argmax_margin(mg, wl)
    wmax = wl.max()
    la = ld(langle)
    stdd = np.full(m_n, np.nan, dtype=LD)
    for m in range(m_n):
        sel = (assoc == m) & (wl[m] / wmax > 0)
        if sel.any():
            mean = la[sel].sum() / sel.sum()
            stdd[m] = np.sqrt(((la[sel] - mean) ** 2).sum() / sel.sum())
    fin = np.sort(stdd[~np.isnan(stdd)])
    mg.note("stdd order: NaN", LD(1) if np.isnan(stdd).sum() <= 1 else LD(0))
    for a, b in zip(fin[:-1], fin[1:]):
        mg.note("stdd order", _rel(a, b, 64 * U * max(abs(a), abs(b))))
    order = sorted(range(m_n), key=lambda m: (not np.isnan(stdd[m]), stdd[m] if not np.isnan(stdd[m]) else 0), reverse=True)
    order = [m for m in order if np.isnan(stdd[m])] + [m for m in order if not np.isnan(stdd[m])]   # argsort()[::-1]: NaN first
    worst = None
    for m in range(m_n):
        cand = order[m]
        nworst = int((assoc == cand).sum())
        mg.note("Nworst > 8", LD(abs(nworst - 8.5)))
        v_ = ld(vi[m])
        with np.errstate(divide="ignore", invalid="ignore"):
            px, py = v_[0] / v_[2], v_[1] / v_[2]                # :557: VP m, not worstVPs[m]
        for x in (px, py):
            mg.note("in image", _rel(abs(x), LD(1), 4 * U))
        if nworst > 8 and (px > -1 and py > -1 and px < 1 and py < 1):
            worst = cand
            break
    out = {"v": vi.copy(), "s": np.array(s, dtype=np.float64), "split": -1, "labels": None, "records": [], "margins": mg}
    if worst is None:
        return out
    idx = np.nonzero(assoc == worst)[0]
    labels = cluster2_reference(ldist_matrix(lp[idx]), mg)
    if labels is None:
        out["labels"] = "disconnected"
        return out
    full = np.full(n_l, -1, dtype=np.int64)
    full[idx] = labels
    out["labels"] = full
    new = []
    for c in range(2):
        rows = idx[labels == c]
        if rows.size < 3:                                        # :592
            continue
        rec = null_vector_reference(l[rows], np.asarray(lw, dtype=np.float64)[rows])
        rec["rows"] = rows
        if rec["vp"][2] < 0:
            rec["vp"] = -rec["vp"]
        new.append(rec)
    out["records"] = new
    if len(new) == 2:
        cphi = np.clip(np.dot(new[0]["vp"], new[1]["vp"]), -1, 1)
        ang = abs(np.arccos(np.clip(abs(cphi), -1, 1)))
        mg.note("min_diff", _rel(ang, LD(min_diff), new[0]["vec_bound"] + new[1]["vec_bound"]))
        if ang > min_diff:
            v2 = np.zeros((m_n + 1, 3), dtype=LD)
            v2[:m_n] = ld(vi)
            v2[worst] = new[0]["vp"]
            v2[m_n] = new[1]["vp"]
            s2 = np.append(ld(s), ld(s)[worst] / 2)
            s2[worst] = ld(s)[worst] / 2
            out.update(v=v2, s=s2, split=int(worst))
    return out


# =============================================================================================================
# merge
# =============================================================================================================
def weight_matrix_reference(p_vl, b_pvl, lw, lsim, bias):
    """weight_matrix (:515-524) in extended precision and the first-order bound of its fp64 evaluation from the bound of
    p_vl: every term is non-negative, so the bound passes through the same operator, plus (N + 8) u of the result and the
    resolution of underflowing products (em_smoother_reference.smooth_reference: the one statement of the formula)."""
    lw_ = ld(lw)
    return smooth_reference(p_vl * lw_[None, :], b_pvl * lw_[None, :], lw, lsim, bias)


def angle_matrix(v):
    v = ld(v)
    d = np.clip(v @ v.T, -1, 1)
    a = np.abs(np.arccos(np.clip(np.abs(d), -1, 1)))
    np.fill_diagonal(a, PI64)
    return a


def merge_reference(vi, s, l, thresh, lw, lsim, wbias, pdfpar, lp, max_stdd=0.01):
    """merge_vps on one slice: dict of v (M', 3), s (M'), kept (indices of the input), rounds (one record per merge
    attempt: j, k, the null-vector record with its row weights r and their bound b_r, s_k and its relative bound, ok)
    and the margins.  From the second round on the restatement continues from its own extended-precision VPs."""
    v = ld(np.asarray(vi, dtype=np.float64)).copy()
    s = ld(s).copy()
    kept = list(range(v.shape[0]))
    mg = Margins()
    rounds = []
    n_l = lp.shape[0]
    while v.shape[0] > 1:
        ang = angle_matrix(v)
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
        e = estep_reference(pdfpar, v.astype(np.float64), lp, s.astype(np.float64))
        s = e["s"].copy()                                        # calc_plv floors s in place (:139)
        w, b_w = weight_matrix_reference(e["p_vl"], e["b_pvl"], lw, lsim, wbias)
        r = w[j] + w[k]
        rec = {"j": j, "k": k, "none": bool(n_l == 0 or r.max() == 0)}
        pq = e["p_vl"][k] + e["p_vl"][j]
        lq = LD(0.5) * (e["lvsq"][:, j] + e["lvsq"][:, k])
        sv, sp = (lq * pq).sum(), pq.sum()
        d_sv = (LD(0.5) * (e["b_lvsq"][:, j] + e["b_lvsq"][:, k]) * pq + lq * (e["b_pvl"][k] + e["b_pvl"][j])).sum()
        d_sp = (e["b_pvl"][k] + e["b_pvl"][j]).sum()
        s_k = sv / sp
        rec["s_k"] = s_k
        rec["rel_s"] = (2 * n_l + 8) * U + 2 * U * (abs(np.log(sv)) + abs(np.log(sp))) + d_sv / sv + d_sp / sp
        s[k] = s_k                                               # :666, before the abort test
        mg.note("s[k] > max_stdd", _rel(s_k, LD(max_stdd), rec["rel_s"] * s_k))
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
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _lines_of(lp):
    """homogeneous lines through the end points, unit norm (what the EM normalises to, :185-186)"""
    n = lp.shape[0]
    a = np.c_[lp[:, :2], np.ones(n)]
    b = np.c_[lp[:, 2:], np.ones(n)]
    return _unit(np.cross(a, b))


def _segments_to(rs, point, n, jitter, centre=None, spread=1.0):
    """n segments whose lines pass the image point ``point`` to within an angle of ``jitter``"""
    mid = rs.uniform(-1, 1, (n, 2)) * spread + (0 if centre is None else np.asarray(centre))
    d = np.asarray(point)[None, :] - mid
    phi = np.arctan2(d[:, 1], d[:, 0]) + rs.uniform(-jitter, jitter, n)
    half = rs.uniform(0.05, 0.2, n)[:, None] * np.c_[np.cos(phi), np.sin(phi)]
    return np.c_[mid - half, mid + half]


def _vps_in_image(rs, m):
    pts = rs.uniform(-0.9, 0.9, (m, 2))
    return _unit(np.c_[pts, np.ones(m)]), pts


COUNT_N = (1, 63, 64, 65, 513)        # 513: one past the workgroup's 512 threads
COUNT_M = (1, 2, 64)


def counts_cases():
    """name -> inputs.  Every (N, M); thresh alternates between the reference's default and the EM's 1.96^2; every other
    case passes a vp_assoc with -1 entries; lweights have zeros; one VP of the M = 2 cases lies at infinity (v[2] == 0)."""
    out = {}
    q = 0
    for n in COUNT_N:
        for m in COUNT_M:
            for seed in range(1000):
                rs = np.random.RandomState(7919 * n + 104729 * m + seed)
                vp, pts = _vps_in_image(rs, m)
                own = rs.randint(0, m, n)
                lp = np.concatenate([_segments_to(rs, pts[own[i]], 1, 0.12) for i in range(n)])
                if m == 2:
                    vp[1] = _unit([0.6, 0.8, 0.0])
                s = rs.uniform(0.5, 2.0, m) * 4e-12
                dist = np.array([[float(lvsq_single(vp[k], lp[i])[0]) for i in range(n)] for k in range(m)])
                metric = 1.0 / (1e-6 + np.nan_to_num(dist, nan=1.0)) * rs.uniform(0.8, 1.2, (m, n))
                lw = rs.uniform(0.1, 1.0, n)
                lw[::5] = 0.0
                thresh = 2.57 if q % 2 == 0 else 1.96 ** 2
                assoc = None
                if q % 2 == 1:
                    assoc = own.astype(np.int64)
                    assoc[::4] = -1
                case = {"vp": vp, "lp": lp, "s": s, "metric": metric, "lweights": lw, "thresh": np.float64(thresh)}
                if assoc is not None:
                    case["vp_assoc"] = assoc
                if counts_reference(vp, lp, s, metric, lw, thresh, assoc)[3].clear():
                    break
            else:
                raise AssertionError("no clear counts case for N = %d, M = %d" % (n, m))
            out["counts_n%d_m%d" % (n, m)] = case
            q += 1
    return out


def _bundle(rs, point, phi0, n, width, jitter):
    """n segments in a cone around direction phi0 seen from ``point``, their lines passing it to within ``jitter``"""
    phi = phi0 + rs.uniform(-width, width, n)
    rad = rs.uniform(0.5, 1.5, n)
    mid = np.asarray(point)[None, :] + rad[:, None] * np.c_[np.cos(phi), np.sin(phi)]
    psi = phi + rs.uniform(-jitter, jitter, n)
    half = rs.uniform(0.05, 0.2, n)[:, None] * np.c_[np.cos(psi), np.sin(psi)]
    return np.c_[mid - half, mid + half]


def _fold_angles(lp):
    """lines_angles (:765-776) restated: the angle against the x axis folded into [0, pi / 2]"""
    d = lp[:, 2:] - lp[:, :2]
    a = np.abs(np.arctan2(d[:, 1], d[:, 0]))
    return np.where(a > np.pi / 2, np.pi - a, a)


SPLIT_SPECS = {
    # name: (M, sizes of the worst VP's two bundles, angle between the bundles, min_diff, worst VP outside the image)
    "split_nworst8": (3, (4, 4), 1.0, 1e-4, False),
    "split_nworst9": (3, (5, 4), 1.0, 1e-4, False),
    "split_7plus2": (3, (7, 2), 1.0, 1e-4, False),
    "split_too_similar": (3, (6, 6), 1.0, 2.0, False),
    "split_quirk557": (3, (6, 6), 0.6, 1e-4, True),
    "split_m63": (63, (6, 6), 1.0, 1e-4, False),
    "split_nworst65": (2, (33, 32), 0.6, 1e-4, False),
    "split_nworst129": (2, (65, 64), 1.0, 1e-4, False),
}


def split_case(name, m_override=None):
    m, sizes, sep, min_diff, outside = SPLIT_SPECS[name]
    if m_override:
        m = m_override
    for seed in range(1000):
        rs = np.random.RandomState(abs(hash_name(name)) % 100000 + seed)
        vp, pts = _vps_in_image(rs, m)
        worst = m - 1 if outside else 0
        if outside:
            pts[worst] = (1.5, 0.2)
            vp[worst] = _unit([1.5, 0.2, 1.0])
        parts, owner = [], []
        phi0 = rs.uniform(0.1, 0.4)
        pa, pb = pts[worst], pts[worst] + rs.uniform(-0.05, 0.05, 2)
        parts += [_bundle(rs, pa, phi0, sizes[0], 0.05, 2e-3), _bundle(rs, pb, phi0 + sep, sizes[1], 0.05, 2e-3)]
        owner += [worst] * (sizes[0] + sizes[1])
        for k in range(m):
            if k == worst:
                continue
            parts.append(_bundle(rs, pts[k], rs.uniform(0, 1.2), 3, 0.002 * (1 + k % 7), 2e-3))
            owner += [k] * 3
        lp = np.concatenate(parts)
        perm = rs.permutation(lp.shape[0])
        lp, owner = lp[perm], np.array(owner)[perm]
        n = lp.shape[0]
        w = rs.uniform(0.0, 0.2, (m, n))
        w[owner, np.arange(n)] = rs.uniform(0.5, 1.0, n)
        lw = rs.uniform(0.2, 1.0, n)
        s = rs.uniform(0.5, 2.0, m) * 1e-6
        case = {"v": vp, "s": s, "lp": lp, "l": _lines_of(lp), "w": w, "lw": lw, "langle": _fold_angles(lp),
                "min_diff": np.float64(min_diff)}
        ref = split_reference(vp, s, lp, case["l"], w, lw, case["langle"], min_diff)
        if ref["margins"].clear() and not isinstance(ref["labels"], str):
            return case
    raise AssertionError("no clear case for " + name)


def hash_name(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def split_cases():
    return {name: split_case(name) for name in SPLIT_SPECS}


MERGE_SPECS = {
    # name: (N, VP layout, thresh, max_stdd, all-zero line weights, merges carried out, what ends the loop)
    "merge_m1": (12, "one", 1e-3, 0.01, False, 0, "one VP"),
    "merge_m2_below": (24, "pair", 1e-3, 0.01, False, 1, "one VP"),
    "merge_m2_above": (24, "pair_far", 1e-3, 0.01, False, 0, "angle"),
    "merge_chain3": (36, "chain", 3e-2, 0.01, False, 2, "angle"),
    "merge_abort": (24, "pair_and_one", 1e-3, 1e-6, False, 0, "max_stdd"),
    "merge_zero_weights": (24, "pair_and_one", 1e-3, 0.01, True, 0, "none"),
    "merge_n1": (1, "pair_and_one", 1e-3, 0.01, False, 1, "angle"),
    "merge_n64": (64, "pair_and_one", 1e-3, 0.01, False, 1, "angle"),
    "merge_n65": (65, "pair_and_one", 1e-3, 0.01, False, 1, "angle"),
}


def merge_outcome(ref):
    """(merges carried out, what ended the loop) of a merge_reference result"""
    rounds = ref["rounds"]
    done = sum(1 for q in rounds if q["ok"])
    if rounds and not rounds[-1]["ok"]:
        return done, "none" if rounds[-1]["none"] else "max_stdd"
    return done, "one VP" if ref["v"].shape[0] == 1 else "angle"


def _grid():
    """pdf_params' means (probability_functions.py:73-80, :92-94): alpha along a row of the map, beta along a column"""
    c = np.linspace(-19.0 / 20 * np.pi / 2, 19.0 / 20 * np.pi / 2, 20)
    means = np.zeros((400, 2))
    means[:, 0] = np.tile(c, 20)
    means[:, 1] = np.repeat(c, 20)
    return means


def _rotate(v, angle, rs):
    t = np.cross(v, rs.normal(size=3))
    t /= np.linalg.norm(t)
    return _unit(np.cos(angle) * v + np.sin(angle) * t)


def merge_case(name, attempt=0):
    """Inputs without lsim and the prior: the recorder adds them from the reference's calc_lsim and pdf_params, and takes
    the first ``attempt`` whose restatement has clear margins and the outcome the spec names."""
    n, layout, thresh, max_stdd, zero_w = MERGE_SPECS[name][:5]
    rs = np.random.RandomState(hash_name(name) % 100000 + attempt)
    base, pts = _vps_in_image(rs, 3)
    if layout == "one":
        v = base[:1]
    elif layout == "pair":
        v = np.stack([base[0], _rotate(base[0], 2e-4, rs)])
    elif layout == "pair_far":
        v = np.stack([base[0], _rotate(base[0], 1e-2, rs)])
    elif layout == "pair_and_one":
        v = np.stack([base[0], base[1], _rotate(base[0], 2e-4, rs)])
    else:
        v = np.stack([base[0], _rotate(base[0], 2e-4, rs), base[1], _rotate(base[0], 5e-4, rs)])
    own = rs.randint(0, 2, n)
    lp = np.concatenate([_segments_to(rs, pts[own[i]], 1, 0.15) for i in range(n)])
    lw = np.zeros(n) if zero_w else rs.uniform(0.2, 1.0, n)
    cnn = rs.rand(20, 20).astype(np.float32) ** 4
    return {"v": v, "s": np.full(v.shape[0], 1e-4), "lp": lp, "l": _lines_of(lp), "lw": lw, "cnn": cnn,
            "thresh": np.float64(thresh), "wbias": np.float64(1.0), "max_stdd": np.float64(max_stdd)}
