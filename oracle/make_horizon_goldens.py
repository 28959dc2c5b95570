"""Run the REFERENCE's calc_horizon.calculate_horizon_and_ortho_vp over a table of seeded vanishing-point sets.

TEST INFRASTRUCTURE, build container only (needs the reference tree; see ref_shim.py).  A sibling of
make_keyword_goldens.py: that one holds the EM to the reference under every keyword, this one does the same for the stage
behind it -- the triplet selection that vpk_horizon_batch runs on the GPU -- at the keywords, VP counts, ties and
degenerate values that the EM results of ordinary scenes never produce.  It writes ONE file of data,

    tests/golden/horizon/horizon_cases.npz   (a directory of its own: the suite's list of single-run golden cases reads
                                              every *.npz directly under tests/golden)
        kind         [n] label of the case (the table below)
        off          [n + 1] rows of case k are vp[off[k]:off[k + 1]], counts[off[k]:off[k + 1]]
        vp, counts   inputs: the 'vp' and 'counts' of an EM result
        maxbest, theta_vmin, theta_z     the three keywords of the call
        raised       [n] '' or the class name of the exception the reference raised (every score NaN: hlin stays None)
        hP1, hP2, zVP, hVP1, hVP2        [n, 3] float64, the first five returned values (zeros where it raised)
        combo, combo_len                 [n, 3] int32 best_combo padded with -1, and its length (3, or 2 below three VPs)
        sens_kw, sens_a, sens_b          keyword sensitivity: cases a and b have the same inputs and differ in that keyword only
        branch_name, branch_case         branch list: which case takes which branch of the scoring (below)
        tie_first, tie_second            [n] triplet indices (itertools.combinations order) of the bit-equal pair of best
                                         scores of the "tie_*" cases, -1 elsewhere


Case table (seeded; `python oracle/make_horizon_goldens.py` reproduces every array of the committed file; the reference's
times are printed, not stored):
  plausible    a zenith within 12 degrees of the vertical, two horizon VPs orthogonal to it and to each other, clutter
               around them and elsewhere, integer counts: M in {3, 4, 5, 10, 19, 20, 21, 33, 47, 64} x maxbest in
               {3, 10, 20, 33, 64} x (theta_vmin, theta_z) in {(pi/10, pi/4) = the default, (pi/6, pi/3), (pi/16, pi/5)}
  sens_*       pairs that differ in one keyword and in the reference's best_combo, two pairs per keyword
  tie_hi/lo    nb >= 13 and a duplicated VP (same vector, same count): two triplets with bit-equal best scores whose indices
               fall into different threads of the kernel (idx % 256); in tie_hi the earlier triplet sits in the
               higher-numbered thread, in tie_lo in the lower.  The reference keeps the first.
  eqcount      counts drawn from three or four values (long runs of equal counts) at M <= 16 and M > 16: the order among
               equals is np.argsort's, and it decides which VPs are among the best and which triplet comes first
  eq_y_*       every score 0 and the first triplet has two (or three) equal |y|: the three-way comparison's else branch
               decides which member is returned as the zenith
  two_zenith / two_central / tilt / zpos    a triplet with the largest counts of the frame that fails exactly ONE of the
               sanity checks (two zenith candidates; two VPs inside the image; a horizon tilted past 30 degrees;
               zenithPos * horPos == -1) and would otherwise have won ("decisive")
  degenerate   VPs with z == 0, y == 0 or both among ordinary ones; a zenith exactly (0, 1, 0); no zenith candidate at
               all (every score 0); every score NaN (the reference raises)
  few          M = 0, 1, 2, and M >= 3 under maxbest = 1, 2
  late_winner  the only triplet that passes the checks is the LAST of the order (index 41 663 of C(64, 3) at maxbest = 64,
               5 455 at maxbest = 33): an orthogonal triple at the three lowest of the nb best counts, every better-supported
               VP a zenith candidate on the horizon's side (two of them in a triplet: two zenith candidates; one with the two
               horizon VPs: zenithPos * horPos == -1).  Thread 0's decode loop runs to the end of the order.

No thresholded decision sits on a rounding edge: `margins` evaluates every triplet of a candidate case in float64 and the
generator redraws the case when, for a triplet that could win (its score with every check passed reaches the best score),
AB / BC / AC lie within 1e-9 of cos(theta_vmin), an |y| within 1e-9 of sin(theta_z), the tilt within 1e-9 of 30 degrees, a
VP's x/z or y/z within 1e-9 of +-1, the horizon's mean height within 1e-9 of 0, or when the two best distinct scores are
closer than 1e-9 relative.  This is a condition on the INPUTS; bit-equal scores (the tie cases) are equal by construction.

Figures of the committed table (printed by a run; tests/test_horizon_cases.py asserts the share):
  202 cases, 20 of them with 33 or more best VPs (C(64, 3) = 41 664 triplets take the reference 9 to 12 s); the winner is not
  triplet 0 on 129 of the 202 = 63.9 % (192 have triplets and a winner at all).  87 s of reference time, 15 s wall on 8
  processes -- with the reference's numCombo3 memoised in memory (run_reference): as written it makes ~1.84^n recursive
  calls, minutes at n = 33 and no end at n = 47 or 64.
  The reference raises on the two "every score NaN" cases (ValueError) and, under today's NumPy, wherever fewer than two VPs
  are scored (UFuncTypeError: the integer hlin of calc_horizon.py:211 / :217 divided in place at :222).
  Branch list: equal |y| -> eq_y_ab, eq_y_bc, eq_y_ac, eq_y_abc; two zenith candidates -> two_zenith; two VPs inside the
  image -> two_central; tilt past 30 degrees -> tilt; zenithPos * horPos == -1 -> zpos (branch_name / branch_case).

Usage:  python oracle/make_horizon_goldens.py [--jobs J] [--out PATH]
"""
import itertools
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

OUT = os.path.join(ROOT, "tests", "golden", "horizon", "horizon_cases.npz")

DEFAULT_TH = (np.pi / 10., np.pi / 4.)
THETAS = (DEFAULT_TH, (np.pi / 6., np.pi / 3.), (np.pi / 16., np.pi / 5.))
PLAUSIBLE_M = (3, 4, 5, 10, 19, 20, 21, 33, 47, 64)
MAXBEST = (3, 10, 20, 33, 64)
EDGE = 1e-9
MAX_TILT = 30 * np.pi / 180
HZ_THREADS = 256                     # threads of horizon_kernel: triplet idx is scored by thread idx % 256


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------------
# every triplet of a case at once (float64, NumPy's roundings or near them: used for margins and labels, never as a result)

def margins(vp, counts, maxbest, theta_vmin, theta_z):
    """None below three best VPs, else a dict: scores [T], the first maximum `win` (-1: every score NaN), `ok_inputs`
    (False: a decision of a triplet that could win sits within EDGE of its threshold, or the two best distinct scores are
    closer than EDGE relative), per-check `decisive` triplets, and the tied best pair."""
    m = vp.shape[0]
    nb = min(maxbest, m)
    if nb < 3:
        return None
    order = np.argsort(counts)[::-1][:nb]
    tri = np.array(list(itertools.combinations(range(nb), 3)))
    idx = order[tri]
    ar = np.arange(len(tri))
    with np.errstate(all="ignore"):
        v = vp[idx]                                                   # T, 3, 3
        c = counts[idx]
        costh, sin_tz = np.cos(theta_vmin), np.sin(theta_z)
        dots = np.stack([np.abs((v[:, 0] * v[:, 1]).sum(1)), np.abs((v[:, 1] * v[:, 2]).sum(1)),
                         np.abs((v[:, 0] * v[:, 2]).sum(1))], 1)
        y = np.abs(v[:, :, 1])
        zen = y > sin_tz
        nz = zen.sum(1)
        last_zen = np.where(zen[:, 2], 2, np.where(zen[:, 1], 1, 0))
        q = vp / vp[:, 2:3]
        inimg = (q[:, 0] <= 1) & (q[:, 0] >= -1) & (q[:, 1] <= 1) & (q[:, 1] >= -1)
        ncen = inimg[idx].sum(1)
        ya, yb, yc = y[:, 0], y[:, 1], y[:, 2]
        role = np.where((ya > yb) & (ya > yc), 0, np.where((yb > ya) & (yb > yc), 1, 2))
        p1, p2 = np.where(role == 0, 1, 0), np.where(role == 2, 1, 2)
        zv, h1, h2 = v[ar, role], v[ar, p1], v[ar, p2]
        c1, c2 = c[ar, p1], c[ar, p2]
        zn = np.hypot(zv[:, 1], zv[:, 0])
        l1, l2 = zv[:, 1] / zn, -zv[:, 0] / zn
        q1, q2 = h1 / h1[:, 2:3], h2 / h2[:, 2:3]
        ez = np.array([0.0, 0.0, 1.0])
        d1, d2 = np.linalg.norm(ez - q1, axis=1), np.linalg.norm(ez - q2, axis=1)
        h3 = ((h1[:, 0] * l2 - h1[:, 1] * l1) / h1[:, 2] * (d2 * c1) + (h2[:, 0] * l2 - h2[:, 1] * l1) / h2[:, 2] * (d1 * c2)) \
            / ((d1 * c2) + (d2 * c1))
        hl0, hl1, hl2 = -l2, l1, h3
        meany = ((hl2 - hl0) / (-hl1) + (-hl2 - hl0) / hl1) / 2
        hvec = q1 - q2
        hn = np.linalg.norm(hvec, axis=1)
        hang = np.arccos(np.abs(hvec[:, 0]) / hn)
        zcand = v[ar, last_zen]
        cosphi = np.abs(((hvec / hn[:, None]) * (zcand / np.linalg.norm(zcand, axis=1)[:, None])).sum(1))
        ortho_if = 1 - np.clip(cosphi, 0, 1)
        ortho = np.where(nz == 1, ortho_if, 0.0)
        g_ang = (dots < costh).all(1)
        g_zen = nz == 1
        g_cen = ncen <= 1
        g_tilt = hang < MAX_TILT
        g_pos = np.where(zv[:, 1] > 0, 1, -1) * np.where(meany < 0, 1, -1) == 1
        wsum = c.sum(1)
        ok = g_ang & g_zen & g_cen & g_tilt & g_pos
        score = ok * wsum * ortho
    finite = ~np.isnan(score)
    win = int(np.nanargmax(score)) if finite.any() else -1
    best = score[win] if win >= 0 else 0.0
    potential = wsum * np.where(g_zen, ortho_if, 1.0)
    could = np.isnan(potential) | (potential >= best * (1 - EDGE))
    # distance of every decision quantity from its threshold (NaN / inf: the comparison is false whatever the rounding)
    dist = [np.abs(dots - costh).min(1), np.abs(y - sin_tz).min(1), np.abs(hang - MAX_TILT), np.abs(meany)]
    edge_vp = np.minimum(np.abs(np.abs(q[:, 0]) - 1), np.abs(np.abs(q[:, 1]) - 1))
    dist.append(edge_vp[idx].min(1))
    near = np.zeros(len(tri), dtype=bool)
    for d in dist:
        near |= np.nan_to_num(d, nan=np.inf) < EDGE
    ok_inputs = not bool((near & could).any())
    vals = np.unique(score[finite])
    if len(vals) > 1 and vals[-1] > 0 and (vals[-1] - vals[-2]) <= EDGE * vals[-1]:
        ok_inputs = False
    others = {"two_zenith": g_ang & g_cen & g_tilt & g_pos & (nz == 2) & (wsum > best),
              "two_central": g_ang & g_zen & g_tilt & g_pos & (ncen == 2) & (wsum * ortho > best),
              "tilt": g_ang & g_zen & g_cen & g_pos & ~g_tilt & (hang >= MAX_TILT) & (wsum * ortho > best),
              "zpos": g_ang & g_zen & g_cen & g_tilt & ~g_pos & (wsum * ortho > best)}
    tied = np.where(score == best)[0] if best > 0 else np.zeros(0, dtype=int)
    return {"score": score, "win": win, "best": best, "ok_inputs": ok_inputs, "decisive": others, "tied": tied,
            "order": order, "tri": tri, "y": y, "role": role}


# ---------------------------------------------------------------------------------------------------------------------
# seeded generators

def ortho_triple(rs, tilt_deg=12.0, zz=(0.05, 0.35), down=None):
    """A zenith near the vertical (z > 0: the horizon lies on the other side of the principal point) and two horizon VPs
    orthogonal to it and to each other."""
    t = np.deg2rad(rs.uniform(-tilt_deg, tilt_deg))
    sgn = -1.0 if (rs.rand() < 0.5 if down is None else down) else 1.0
    zen = unit([np.sin(t), sgn * np.cos(t), rs.uniform(*zz)])
    u = unit(np.cross(zen, [0.0, 0.0, 1.0]))
    w = np.cross(zen, u)
    phi = np.deg2rad(rs.uniform(20, 70))
    h1 = np.cos(phi) * u + np.sin(phi) * w
    h2 = -np.sin(phi) * u + np.cos(phi) * w
    h1, h2 = h1 * np.sign(h1[2]), h2 * np.sign(h2[2])
    return np.stack([zen, h1, h2])


def plausible(rs, m, n_triples=1, count_values=None, **kw):
    """m VPs: orthogonal triples, clutter near them (5-25 degrees off) and anywhere on the sphere; integer counts."""
    base = np.concatenate([np.zeros((0, 3))] + [ortho_triple(rs, **kw) for _ in range(n_triples)])[:m]
    rows = [base]
    k = m - len(base)
    if k > 0:
        anywhere = unit(rs.normal(size=(k, 3)))
        if len(base):
            near = base[rs.randint(0, len(base), k)]
            off = unit(rs.normal(size=(k, 3))) * np.tan(np.deg2rad(rs.uniform(5, 25, (k, 1))))
            anywhere = np.where(rs.rand(k, 1) < 0.5, unit(near + off), anywhere)
        rows.append(anywhere)
    vp = np.concatenate(rows)
    if count_values is None:
        counts = np.concatenate([rs.randint(10, 60, len(base)), rs.randint(3, 50, k)]).astype(np.float64)
    else:
        counts = rs.choice(count_values, m).astype(np.float64)
    p = rs.permutation(m)
    return vp[p], counts[p]


def draw(rs, make, accept, tries=20000):
    """First drawn case that keeps its decisions off the rounding edges and that `accept` takes."""
    for _ in range(tries):
        case = make(rs)
        if accept(case):
            return case
    raise RuntimeError("no acceptable case in %d draws" % tries)


def clean(vp, counts, settings):
    for mb, tv, tz in settings:
        a = margins(vp, counts, mb, tv, tz)
        if a is not None and not a["ok_inputs"]:
            return False
    return True


def winner_set(vp, counts, mb, tv, tz):
    a = margins(vp, counts, mb, tv, tz)
    if a is None or a["win"] < 0:
        return None
    return tuple(a["order"][a["tri"][a["win"]]])


def build_table():
    """[(kind, vp, counts, maxbest, theta_vmin, theta_z)], sensitivity pairs, branch list, tie indices."""
    cases, sens, branches, ties = [], [], [], {}

    def add(kind, vp, counts, mb, tv, tz):
        cases.append((kind, np.ascontiguousarray(vp, dtype=np.float64).reshape(-1, 3),
                      np.ascontiguousarray(counts, dtype=np.float64), int(mb), float(tv), float(tz)))
        return len(cases) - 1

    # plausible frames: the full cross
    for m in PLAUSIBLE_M:
        for mb in MAXBEST:
            for ti, (tv, tz) in enumerate(THETAS):
                rs = np.random.RandomState(100000 + 1000 * m + 10 * mb + ti)
                vp, cn = draw(rs, lambda r: plausible(r, m, n_triples=1 + (m >= 10)),
                              lambda cs: clean(cs[0], cs[1], [(mb, tv, tz)]))
                add("plausible", vp, cn, mb, tv, tz)

    # keyword sensitivity: the same inputs under two values of ONE keyword, different winners
    variants = {"maxbest": [((10,) + DEFAULT_TH, (20,) + DEFAULT_TH), ((3,) + DEFAULT_TH, (10,) + DEFAULT_TH)],
                "theta_vmin": [((20, np.pi / 10., np.pi / 4.), (20, np.pi / 6., np.pi / 4.)),
                               ((10, np.pi / 16., np.pi / 4.), (10, np.pi / 10., np.pi / 4.))],
                "theta_z": [((20, np.pi / 10., np.pi / 4.), (20, np.pi / 10., np.pi / 3.)),
                            ((10, np.pi / 10., np.pi / 5.), (10, np.pi / 10., np.pi / 4.))]}
    for ki, (kw, pairs) in enumerate(variants.items()):
        for pi_, (sa, sb) in enumerate(pairs):
            rs = np.random.RandomState(200000 + 10 * ki + pi_)

            def differs(cs, sa=sa, sb=sb):
                if not clean(cs[0], cs[1], [sa, sb]):
                    return False
                wa, wb = winner_set(cs[0], cs[1], *sa), winner_set(cs[0], cs[1], *sb)
                return wa is not None and wb is not None and wa != wb
            vp, cn = draw(rs, lambda r: plausible(r, 24, n_triples=3, tilt_deg=25.0, zz=(0.05, 0.7)), differs)
            sens.append((kw, add("sens_" + kw, vp, cn, *sa), add("sens_" + kw, vp, cn, *sb)))

    # exact score ties across threads
    for kind, want_hi in (("tie_hi", True), ("tie_lo", False)):
        rs = np.random.RandomState(300000 + want_hi)

        def make_tie(r):
            m = int(r.randint(13, 24))
            vp, cn = plausible(r, m, n_triples=1)
            a = margins(vp, cn, 64, *DEFAULT_TH)
            if a["win"] < 0 or a["best"] <= 0:
                return None
            members = a["order"][a["tri"][a["win"]]]
            dup = members[r.randint(3)]
            return np.concatenate([vp, vp[dup:dup + 1]]), np.concatenate([cn, cn[dup:dup + 1]])

        def accept_tie(cs, want_hi=want_hi):
            if cs is None or not clean(cs[0], cs[1], [(64,) + DEFAULT_TH]):
                return False
            a = margins(cs[0], cs[1], 64, *DEFAULT_TH)
            t = a["tied"]
            if len(t) != 2 or max(t) < HZ_THREADS or t[0] % HZ_THREADS == t[1] % HZ_THREADS:
                return False
            return (t[0] % HZ_THREADS > t[1] % HZ_THREADS) == want_hi
        vp, cn = draw(rs, make_tie, accept_tie)
        k = add(kind, vp, cn, 64, *DEFAULT_TH)
        ties[k] = tuple(int(t) for t in margins(vp, cn, 64, *DEFAULT_TH)["tied"])

    # runs of equal counts on both sides of NumPy's small-array threshold
    for m in (8, 16, 17, 40, 64):
        for mb in (10, 20):
            rs = np.random.RandomState(400000 + 100 * m + mb)
            vals = (6, 9, 14) if m < 30 else (5, 8, 11, 17)
            vp, cn = draw(rs, lambda r: plausible(r, m, n_triples=2, count_values=vals),
                          lambda cs: clean(cs[0], cs[1], [(mb,) + DEFAULT_TH]))
            add("eqcount", vp, cn, mb, *DEFAULT_TH)
    rs = np.random.RandomState(400001)
    vp, cn = draw(rs, lambda r: plausible(r, 30, n_triples=2, count_values=(7,)),
                  lambda cs: clean(cs[0], cs[1], [(20,) + DEFAULT_TH]))
    add("eqcount", vp, cn, 20, *DEFAULT_TH)                      # all counts equal

    # equal |y| in the first triplet of a frame without a zenith candidate (every score 0)
    def mirror(v):
        return v * np.array([-1.0, 1.0, 1.0])
    flat = [unit([0.6, 0.3, 0.7]), unit([-0.2, 0.1, 0.9]), unit([0.9, -0.25, 0.3]), unit([0.3, 0.2, -0.8])]
    a_, b_ = flat[0], mirror(flat[0])
    lesser = unit([0.5, 0.1, 0.8])
    for kind, first3 in (("eq_y_ab", [a_, b_, lesser]), ("eq_y_bc", [lesser, a_, b_]), ("eq_y_ac", [a_, lesser, b_]),
                         ("eq_y_abc", [a_, b_, a_ * np.array([1.0, -1.0, 1.0])])):
        vp = np.stack(first3 + flat[1:])
        cn = np.array([30.0, 25.0, 20.0, 9.0, 8.0, 7.0])
        a = margins(vp, cn, 10, *DEFAULT_TH)
        assert a["ok_inputs"] and a["best"] == 0 and a["win"] == 0, kind
        branches.append(("equal_abs_y", add(kind, vp, cn, 10, *DEFAULT_TH)))

    # a top-count triplet that fails exactly one sanity check and would otherwise have won
    def spoiled(kind):
        def make(r):
            vp, cn = plausible(r, 12, n_triples=1)
            t = ortho_triple(r, down=False)
            if kind == "two_zenith":                # a second zenith candidate in place of a horizon VP
                t[2] = unit([r.uniform(-0.7, 0.7), r.choice([-1.0, 1.0]) * r.uniform(0.72, 0.9), r.uniform(0.15, 0.6)])
            elif kind == "two_central":             # both horizon VPs inside the image
                t[1], t[2] = unit([r.uniform(0.3, 0.8), r.uniform(-0.3, -0.1), 1.0]), unit([r.uniform(-0.8, -0.3), r.uniform(-0.3, -0.1), 1.0])
            elif kind == "tilt":                    # the whole triple rotated about the optical axis
                ang = np.deg2rad(r.uniform(33, 40))
                rot = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
                t = t @ rot.T
            elif kind == "zpos":                    # the zenith's vector negated: the same point, on the horizon's side
                t[0] = -t[0]
            return np.concatenate([vp, t]), np.concatenate([cn, [90.0, 80.0, 70.0]])

        def accept(cs):
            if not clean(cs[0], cs[1], [(20,) + DEFAULT_TH]):
                return False
            a = margins(cs[0], cs[1], 20, *DEFAULT_TH)
            return a["best"] > 0 and a["win"] != 0 and bool(a["decisive"][kind][0])     # triplet 0: the three largest counts
        return make, accept
    for ki, kind in enumerate(("two_zenith", "two_central", "tilt", "zpos")):
        rs = np.random.RandomState(500000 + ki)
        vp, cn = draw(rs, *spoiled(kind))
        branches.append((kind, add(kind, vp, cn, 20, *DEFAULT_TH)))

    # degenerate values
    def with_special(specials, seed, m=9, top=False):
        def make(r):
            vp, cn = plausible(r, m, n_triples=1)
            sp = np.array(specials, dtype=np.float64)
            sc = r.randint(60, 90, len(sp)).astype(np.float64) if top else r.randint(5, 40, len(sp)).astype(np.float64)
            return np.concatenate([sp, vp]), np.concatenate([sc, cn])
        return draw(np.random.RandomState(seed), make, lambda cs: clean(cs[0], cs[1], [(20,) + DEFAULT_TH]))
    inf_vps = [[1.0, 0.0, 0.0], unit([0.6, 0.8, 0.0]), unit([0.8, 0.0, 0.6]), unit([-0.3, 0.0, 0.9])]   # y = z = 0; z = 0; y = 0 (twice)
    add("degenerate_mixed", *with_special(inf_vps, 600001), 20, *DEFAULT_TH)
    add("degenerate_mixed_top", *with_special(inf_vps, 600002, top=True), 20, *DEFAULT_TH)
    add("degenerate_mixed_top", *with_special(inf_vps[:2], 600003, top=True), 10, *DEFAULT_TH)
    for seed in (600004, 600005):                                 # the zenith exactly (0, 1, 0), the horizon just below the centre
        r = np.random.RandomState(seed)

        def make(r):
            phi = np.deg2rad(r.uniform(25, 65))
            tri3 = np.stack([[0.0, 1.0, 0.0], unit([np.cos(phi), -r.uniform(0.05, 0.2), np.sin(phi)]),
                             unit([-np.sin(phi), -r.uniform(0.05, 0.2), np.cos(phi)])])
            vp, cn = plausible(r, 7, n_triples=0)
            return np.concatenate([tri3, vp]), np.concatenate([[50.0, 45.0, 40.0], cn])
        add("degenerate_zenith_exact", *draw(r, make, lambda cs: clean(cs[0], cs[1], [(20,) + DEFAULT_TH])), 20, *DEFAULT_TH)
    r = np.random.RandomState(600006)                             # no zenith candidate: every triplet scores 0

    def make_flat(r):
        v = unit(r.normal(size=(14, 3)) * np.array([1.0, 0.3, 1.0]))
        return v, r.randint(3, 50, 14).astype(np.float64)
    for mb in (10, 64):
        vp, cn = draw(r, make_flat, lambda cs: np.abs(cs[0][:, 1]).max() < 0.6 and clean(cs[0], cs[1], [(mb,) + DEFAULT_TH]))
        assert margins(vp, cn, mb, *DEFAULT_TH)["best"] == 0
        add("degenerate_all_zero", vp, cn, mb, *DEFAULT_TH)
    # every score NaN: one zenith candidate per triplet and every VP at infinity (inf - inf in the horizon vector)
    add("degenerate_all_nan", np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], unit([0.8, 0.6, 0.0])]), np.array([9.0, 8.0, 7.0]),
        10, *DEFAULT_TH)
    add("degenerate_all_nan", np.array([unit([0.1, -0.99, 0.0]), [1.0, 0.0, 0.0], unit([0.9, 0.4, 0.0]), unit([0.2, 0.9, 0.3])]),
        np.array([9.0, 8.0, 7.0, 2.0]), 3, *DEFAULT_TH)

    # fewer than three VPs to choose from
    r = np.random.RandomState(700000)
    for m, mb in ((0, 10), (1, 10), (2, 10), (2, 20), (1, 64), (5, 1), (5, 2), (30, 2)):
        add("few", unit(r.normal(size=(m, 3))) if m else np.zeros((0, 3)), r.randint(3, 40, m).astype(np.float64), mb, *DEFAULT_TH)

    # the winner is the last triplet of the order
    for seed, m, mb in ((800001, 64, 64), (800002, 40, 33)):
        nb = min(m, mb)

        def make_late(r, m=m, nb=nb):
            t = ortho_triple(r, down=False)
            spoil = np.stack([-ortho_triple(r, tilt_deg=25.0, down=False)[0] for _ in range(m - 3)])
            vp = np.concatenate([spoil[:nb - 3], t[1:], t[:1], spoil[nb - 3:]])
            return vp, np.arange(300, 300 - 2 * m, -2).astype(np.float64)

        def accept_late(cs, mb=mb, nb=nb):
            if not clean(cs[0], cs[1], [(mb,) + DEFAULT_TH]):
                return False
            a = margins(cs[0], cs[1], mb, *DEFAULT_TH)
            return a["best"] > 0 and a["win"] == len(a["tri"]) - 1 and (a["score"] > 0).sum() == 1
        add("late_winner", *draw(np.random.RandomState(seed), make_late, accept_late), mb, *DEFAULT_TH)
    return cases, sens, branches, ties


# ---------------------------------------------------------------------------------------------------------------------
# the reference

_REF = {}


def run_reference(case):
    if not _REF:
        warnings.filterwarnings("ignore")
        from ref_shim import load_reference
        _REF["ch"] = load_reference(["calc_horizon"])["calc_horizon"]
        # numCombo3 (calc_horizon.py:3-8) calls itself three times per level: ~1.84^n calls, minutes at n = 33 and no end at
        # n = 47.  It is a pure function of n; memoising it in memory changes no value and lets the reference run at 64.
        import functools
        _REF["ch"].numCombo3 = functools.lru_cache(maxsize=None)(_REF["ch"].numCombo3)
    kind, vp, counts, mb, tv, tz = case
    t0 = time.time()
    out = {"raised": "", "hP1": np.zeros(3), "hP2": np.zeros(3), "zVP": np.zeros(3), "hVP1": np.zeros(3), "hVP2": np.zeros(3),
           "combo": np.full(3, -1, np.int32), "combo_len": 0}
    with np.errstate(all="ignore"):
        try:
            res = _REF["ch"].calculate_horizon_and_ortho_vp({"vp": vp.copy(), "counts": counts.copy()}, maxbest=mb,
                                                            theta_vmin=tv, theta_z=tz)
            for k, v in zip(("hP1", "hP2", "zVP", "hVP1", "hVP2"), res[:5]):
                out[k] = np.asarray(v, dtype=np.float64)
            combo = np.asarray(res[5]).ravel()
            out["combo"][:len(combo)] = combo
            out["combo_len"] = len(combo)
        except Exception as e:                  # every score NaN: hlin is still None at calc_horizon.py:220
            out["raised"] = type(e).__name__
    out["ref_seconds"] = time.time() - t0
    return out


def main(argv):
    from concurrent.futures import ProcessPoolExecutor
    jobs, out_path = 8, OUT
    while argv:
        a = argv.pop(0)
        if a == "--jobs":
            jobs = int(argv.pop(0))
        elif a == "--out":
            out_path = argv.pop(0)
        else:
            raise SystemExit(__doc__)
    t0 = time.time()
    cases, sens, branches, ties = build_table()
    t_table = time.time() - t0
    order = sorted(range(len(cases)), key=lambda k: -min(cases[k][3], cases[k][1].shape[0]))      # the long ones first
    with ProcessPoolExecutor(max_workers=jobs) as pool:
        done = list(pool.map(run_reference, [cases[k] for k in order]))
    res = [None] * len(cases)
    for k, r in zip(order, done):
        res[k] = r
    nontrivial = 0
    for k, ((kind, vp, counts, mb, tv, tz), r) in enumerate(zip(cases, res)):
        a = margins(vp, counts, mb, tv, tz)
        if a is None or r["raised"]:
            # the reference raises when every score is NaN, and below two best VPs (an integer hlin divided in place, :220-223)
            assert r["raised"] == "" or a is None or a["win"] < 0, (k, kind, vp.shape, mb, r["raised"])
            continue
        # the vectorised evaluation is only trusted because it names the reference's winner on every case
        assert tuple(r["combo"]) == tuple(a["order"][a["tri"][a["win"]]]), (k, kind)
        nontrivial += a["win"] != 0
        if k in ties:
            assert a["win"] == ties[k][0], (k, kind)
    for kw, a, b in sens:
        assert not np.array_equal(res[a]["combo"], res[b]["combo"]), (kw, a, b)
    off = np.concatenate([[0], np.cumsum([c[1].shape[0] for c in cases])]).astype(np.int64)
    out = {"kind": np.array([c[0] for c in cases]), "off": off,
           "vp": np.concatenate([c[1] for c in cases]), "counts": np.concatenate([c[2] for c in cases]),
           "maxbest": np.array([c[3] for c in cases], dtype=np.int32),
           "theta_vmin": np.array([c[4] for c in cases]), "theta_z": np.array([c[5] for c in cases]),
           "raised": np.array([r["raised"] for r in res]),
           "combo": np.stack([r["combo"] for r in res]), "combo_len": np.array([r["combo_len"] for r in res], dtype=np.int32),
           "sens_kw": np.array([s[0] for s in sens]), "sens_a": np.array([s[1] for s in sens], dtype=np.int32),
           "sens_b": np.array([s[2] for s in sens], dtype=np.int32),
           "branch_name": np.array([b[0] for b in branches]), "branch_case": np.array([b[1] for b in branches], dtype=np.int32),
           "tie_first": np.array([ties.get(k, (-1, -1))[0] for k in range(len(cases))], dtype=np.int32),
           "tie_second": np.array([ties.get(k, (-1, -1))[1] for k in range(len(cases))], dtype=np.int32)
           }
    for k in ("hP1", "hP2", "zVP", "hVP1", "hVP2"):
        out[k] = np.stack([r[k] for r in res])
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    tmp = out_path + ".tmp.npz"
    np.savez_compressed(tmp, **out)
    os.replace(tmp, out_path)
    big = sum(1 for c in cases if min(c[3], c[1].shape[0]) >= 33)
    with_triplets = sum(1 for c, r in zip(cases, res) if min(c[3], c[1].shape[0]) >= 3 and not r["raised"])
    print("%d cases (%d with >= 33 best VPs), winner is not triplet 0 on %d = %.1f%% of all cases (%d have triplets and a "
          "winner); %.1f s of reference time, %.1f s for the table, %.1f s wall -> %s (%d bytes)" % (
              len(cases), big, nontrivial, 100.0 * nontrivial / len(cases), with_triplets,
              sum(r["ref_seconds"] for r in res), t_table, time.time() - t0, out_path, os.path.getsize(out_path)))
    for name, k in branches:
        print("  branch %-12s case %d (%s)" % (name, k, cases[k][0]))


if __name__ == "__main__":
    main(sys.argv[1:])
