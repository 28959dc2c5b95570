"""Extended-precision reference of the EM's smoother (weight_matrix, vp_localisation.py:515-524; smooth() in
csrc/em_device.hpp), its first-order bound, a restatement of the dispatch that names the kernel a call takes, and the
shared case generators of tests/test_em_smoother.py (CPU: the float64 NumPy expression and the host build of the device
source) and tests/test_gpu_em_smoother.py (the HIP kernels).  CPU only.

    w[m][k] = (w_[m][k] + bias lweight[k] sum_j w_[m][j] lsim[j][k]) / (1 + bias lweight[k] sum_j lsim[j][k]),
    w_[m][j] = p_vl[m][j] lweight[j]

No bar below is fitted to what a kernel returns.  Every generated operand is non-negative, so the bound of the operands
passes through the same operator and no cancellation term is needed.
"""
import zlib

import numpy as np

from em_phase_reference import LD, U, TINY, ld, _ratio, _note, WORST, estep_case   # noqa: F401

MT = 8                          # VP tile of the smoothing kernels
RS_RED_DOUBLES = 4 * 16 * 9     # smooth_rows' reduction scratch per wave
RS_PANEL_FLAG = 0x100
DEFAULT_BUDGET = 18880          # doubles of LDS the workgroup plans with when vpk_em_set_lds_panel is 0
BIASES = (1.0, 0.001, 0.0)


# =============================================================================================================
# the formula and its bound
# =============================================================================================================
def smooth_reference(w_, b_w, lw, lsim, bias):
    """weight_matrix on the operands w_ = p_vl * lweight (M, N), in extended precision, and the first-order bound of an
    fp64 evaluation whose operands are off by at most b_w:

      the operand bound through the same non-negative operator
      + (N + 8) u |w|        N: a sum of N non-negative products in any order; 8: q * lw, bias * lw, the two products and
                             the sum of den, the final multiply-add and the division
      + (N + 2) 2^-1074      the resolution of products that underflow
    """
    w_, b_w, lw_, ls = ld(w_), ld(b_w), ld(lw), ld(lsim)
    n = lw_.shape[0]
    with np.errstate(all="ignore"):
        blw = LD(bias) * lw_
        den = 1 + blw * ls.sum(axis=0)
        w = (w_ + blw[None, :] * (w_ @ ls)) / den[None, :]
        b = (b_w + blw[None, :] * (b_w @ np.abs(ls))) / den[None, :] + (n + 8) * U * np.abs(w) + (n + 2) * TINY
    return w, b


def numpy_expression(p_vl, lw, lsim, bias):
    """The reference's expression in float64 NumPy (one matrix product instead of its loops)."""
    with np.errstate(all="ignore"):
        w_ = p_vl * lw[None, :]
        return (w_ + bias * lw[None, :] * (w_ @ lsim)) / (1 + bias * lw * lsim.sum(axis=0))[None, :]


def check_smooth(got, w, bar, label):
    """got within bar of the extended reference w where that is finite, NaN exactly where it is NaN.  Returns and records
    (WORST, per label) the worst error / bar."""
    got = np.asarray(got, dtype=np.float64)
    nan = np.isnan(w.astype(np.float64)) | np.isnan(bar.astype(np.float64))
    assert np.array_equal(np.isnan(got), nan), "%s: the NaN pattern differs from the reference's" % label
    assert np.isfinite(got[~nan]).all(), "%s: an infinite result" % label
    r = _ratio(np.abs(ld(got) - w)[~nan], bar[~nan]) if (~nan).any() else 0.0
    _note("smooth " + label, r)
    assert r <= 1.0, "%s: error / bar = %.3g" % (label, r)
    return r


# =============================================================================================================
# which kernel a call takes: smooth_plan() and smooth_dispatch() of csrc/em_device.hpp, restated
# =============================================================================================================
def rs_jchunk(n):
    return (n + 7) >> 3


def rs_sstride(jch, w):
    q = jch * w
    return q + ((16 - q) & 31)


def rs_panel_doubles(jch, w):
    return 8 * rs_sstride(jch, w) + 32


def rs_wfit(n, wt):
    jch = rs_jchunk(n)
    for w in (32, 24, 16, 8):
        if rs_panel_doubles(jch, w) + 8 * RS_RED_DOUBLES <= wt:
            return w
    return 0


def is_direct(n):
    colw = 128 if n > 64 else 64
    return ((n + colw - 1) // colw) % 8 == 0


def smooth_plan(n, m, wt, mode):
    wp = (m + MT - 1) // MT * MT
    rows_ok = mode != 1
    direct = is_direct(n)
    if m <= 32:
        if rows_ok and not direct and rs_panel_doubles(rs_jchunk(n), wp) + 8 * RS_RED_DOUBLES <= wt:
            return 2
        if n * wp <= wt:
            return 1
    if rows_ok and not direct and (wt // n) // MT >= 1 and rs_wfit(n, wt) >= MT:
        return 3
    return 0


def sparse_fits(n, wt, mode):
    c = (n + 63) // 64
    ldw = (c + 1) // 2 * 128
    return mode == 2 and c <= 7 and (3 if c <= 6 else 2) * 16 * ldw <= wt


def expected_info(n, m, wt, mode, finite=True, estep=True):
    """What the hook's info must read for this shape, budget and setting (estep=False: the flag of a call without an
    E-step, vpk_weight_matrix)."""
    plan = smooth_plan(n, m, wt, mode)
    wp = (m + MT - 1) // MT * MT
    flag = (RS_PANEL_FLAG + wp if plan == 2 else wp if plan == 1 else 0) if estep else 0
    width = rs_wfit(n, wt) if plan == 3 else min(32, (wt // n) // MT * MT)
    return [plan, flag, int(sparse_fits(n, wt, mode) and finite), width]


def staged(info):
    """The same info for a call in which no E-step ran (vpk_weight_matrix): no panel flag."""
    out = [int(x) for x in info]
    out[1] = 0
    return out


class Path(object):
    def __init__(self, kernels, handed, width):
        self.kernels, self.handed, self.width = tuple(kernels), bool(handed), int(width)

    def __repr__(self):
        return "%s%s" % ("+".join(self.kernels), " (panel handed over)" if self.handed else "")


def path_of(n, m, wt_doubles, mode, info):
    """The kernels smooth_dispatch runs, pass by pass, from the hook's info (plan, the E-step's panel flag, whether the
    sparse smoother applies, the pass width): 'rows<NT>', 'sparse<C>', 'full<NT,C>:sliced' / 'full<NT,C>:direct' or
    'blocks<C>'; .handed tells whether the smoother consumed the E-step's panel; .width is VPs per pass.  The plan and the
    width are restated here from (n, m, budget, setting) as well and must agree with the device's."""
    plan, flag, sparse, width = (int(x) for x in info)
    want = expected_info(n, m, wt_doubles, mode, finite=True, estep=True)
    assert plan == want[0] and width == want[3], "smooth_plan restated: %s, the device says %s" % (want, list(info))
    assert flag in (0, want[1]), "the E-step's panel flag is %#x, its plan %d asks for %#x" % (flag, plan, want[1])
    assert sparse <= want[2]

    def passes(w):
        return [min(m - m0, w) for m0 in range(0, m, w)]

    if flag >= RS_PANEL_FLAG or plan in (2, 3):
        if sparse:
            return Path(["sparse<%d>" % ((n + 63) // 64)] * len(passes(32)), False, 32)
        wpass = width if plan == 3 else 32
        return Path(["rows<%d>" % ((mm + 7) // 8) for mm in passes(wpass)], flag >= RS_PANEL_FLAG, wpass)
    c = 2 if n > 64 else 1
    if width >= MT:
        kind = "direct" if is_direct(n) else "sliced"
        return Path(["full<%d,%d>:%s" % ((mm + 7) // 8, c, kind) for mm in passes(width)], flag != 0, width)
    return Path(["blocks<%d>" % c], False, 0)


# =============================================================================================================
# case generators, seeded by shape.  Each returns p_vl (M, N), lweight (N), lsim (N, N), all float64 and >= 0
# =============================================================================================================
def _seed(tag, n, m):
    return zlib.crc32(("%s %d %d" % (tag, n, m)).encode()) & 0x7fffffff


def sparse_case(n, m):
    """Production-like operands: 83 % of p_vl exactly zero (the rest 1e-300 .. 1), one VP row and the last line's column
    entirely zero, 10 % of lweight exactly zero (the rest in (0, 0.4)), an ASYMMETRIC lsim with 30 % exact zeros, a zero
    diagonal and magnitudes 1e-12 .. 1."""
    rs = np.random.RandomState(_seed("sparse", n, m))
    p_vl = 10.0 ** rs.uniform(-300, 0, (m, n))
    p_vl[rs.uniform(size=(m, n)) < 0.83] = 0.0
    if m >= 2:
        p_vl[m // 2] = 0.0
    if n >= 2:
        p_vl[:, n - 1] = 0.0
    lw = rs.uniform(0.0, 0.4, n)
    lw[lw == 0.0] = 0.2
    lw[rs.uniform(size=n) < 0.10] = 0.0
    lsim = 10.0 ** rs.uniform(-12, 0, (n, n))
    lsim[rs.uniform(size=(n, n)) < 0.30] = 0.0
    np.fill_diagonal(lsim, 0.0)
    return {"p_vl": p_vl, "lweight": lw, "lsim": lsim}


def coded_case(n, m):
    """Small integers times powers of two, functions of (m, j) and (j, k): every product w_[m][j] lsim[j][k] and every
    partial sum of them -- and every partial sum of a column of lsim -- is exact in fp64 in any order (integers below
    2^10, at most three binary exponents apart, N <= 1025: sums below 2^33), so a dropped, duplicated, transposed or
    misplaced row, column, VP or slice changes the exact sum.  lweight is a power of two, lsim is asymmetric."""
    mm, jj = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    a = 1 + (7 + 131 * mm + 37 * jj + (mm * jj) % 11 + (jj * jj) % 13) % 1008
    p_vl = a * 2.0 ** -10 * 2.0 ** -(mm % 5)
    lw = 2.0 ** -(1 + np.arange(n) % 3)
    j2, kk = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    c = 1 + (3 + 17 * j2 + 59 * kk + (j2 * j2 * kk) % 19 + (kk % 7) * (j2 % 5)) % 1012
    lsim = c * 2.0 ** -14
    return {"p_vl": p_vl.astype(np.float64), "lweight": lw, "lsim": lsim.astype(np.float64)}


def coded_bar(w):
    """8 u |w|: the sums are exact, only den (bias * lw, the product, 1 +) and the final expression round."""
    return 8 * U * np.abs(w)


def edge_slice_case(n, m):
    """Coded values; VP 0's only non-zero operand sits in the last existing row (line n - 1), VP 1's in the first row of
    slice 1 (line ceil(n / 8)).  At n = 9 the slices are two rows long: slice 4 holds one line, slices 5 .. 7 none."""
    case = coded_case(n, m)
    jch = rs_jchunk(n)
    keep = case["p_vl"].copy()
    case["p_vl"][0] = 0.0
    case["p_vl"][0, n - 1] = keep[0, n - 1]
    if m >= 2 and jch < n:
        case["p_vl"][1] = 0.0
        case["p_vl"][1, jch] = keep[1, jch]
    return case


NONFINITE = ("inf", "nan", "overflow")


def nonfinite_case(n, m, kind):
    """sparse_case with one fault in column k of lsim (returned as case['k']):
      inf       lsim[j][k] = +Inf in a row j whose operands w_[:, j] are all zero: 0 * Inf
      nan       lsim[j][k] = NaN
      overflow  two entries of 1.5e308 whose sum overflows; k is a column with lweight[k] = 0, where den = 1 + 0 * Inf is
                NaN (with a positive lweight the column would be finite / Inf = 0 in NumPy too and say nothing about NaN)
    """
    assert n >= 3 and kind in NONFINITE
    case = sparse_case(n, m)
    lw, lsim = case["lweight"], case["lsim"]
    rs = np.random.RandomState(_seed(kind, n, m))
    if kind == "overflow":
        zero = np.flatnonzero(lw == 0.0)
        if zero.size == 0:
            lw[n // 2] = 0.0
            zero = np.array([n // 2])
        k = int(zero[rs.randint(zero.size)])
        rows = [j for j in range(n) if j != k]
        for j in (rows[0], rows[-1]):
            lsim[j, k] = 1.5e308
    else:
        j = int(rs.randint(n))
        if kind == "inf":
            case["p_vl"][:, j] = 0.0
        k = int((j + 1 + rs.randint(max(n - 1, 1))) % n)
        lsim[j, k] = np.inf if kind == "inf" else np.nan
    case["k"] = k
    return case


def handoff_case(n, m, degenerate=False):
    """Inputs of the hook: em_phase_reference.estep_case(n, m) for the E-step, lweight and lsim of sparse_case(n, m) (zeros
    included, no lweight equal to 1).  estep_case's zero-length segment and its line through a VP's image point make p_vl
    NaN for their lines, and one NaN operand makes EVERY w NaN: they stay only with degenerate=True."""
    e = estep_case(n, m, midpoint_line=degenerate)
    if not degenerate and n >= 7:
        e["lp"][2, 2:] = e["lp"][2, :2] + np.array([0.015625, -0.03125])
    sp = sparse_case(n, m)
    e["lweight"], e["lsim"] = sp["lweight"], sp["lsim"]
    e["bias"] = 1.0 if (n + m) % 3 else 0.001
    return e


# =============================================================================================================
# shapes (N, M).  The budget is in doubles (vpk_em_set_lds_panel; None = the default, DEFAULT_BUDGET)
# =============================================================================================================
ROWS_N = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129)
ROWS_M = (1, 8, 9, 16, 17, 24, 25, 32)
# every N once, every M (at least) once, the four corners of the N x M grid twice
ROWS_SHAPES = [(nn, ROWS_M[i % 8]) for i, nn in enumerate(ROWS_N)] + [(1, 32), (129, 1), (129, 32), (1, 1)]
SECOND_PASS_SHAPES = [(65, 33), (129, 40), (257, 64)]
SPARSE_SHAPES = [(nn, 20) for nn in (64, 65, 129, 193, 257, 321, 385, 448, 449)]
FULL_EDGE_SHAPES = [(896, 8), (897, 8), (1024, 9), (1025, 8)]
FULL_C_SHAPES = [(nn, mm) for nn in (64, 65) for mm in (8, 9, 17, 25)]
# CPU shapes of the issue (the float64 expression against the bound)
CPU_SHAPES = [(1, 1), (7, 3), (9, 8), (17, 17), (63, 25), (64, 32), (65, 33), (129, 40), (257, 64), (449, 20), (897, 8), (1025, 8)]
LIMITED = [(65, 33, 6144), (129, 40, 6144), (129, 40, 2048), (128, 24, 2048), (65, 33, 2048), (16, 9, 96), (129, 40, 96), (9, 8, 64)]


def handoff_reference(case):
    """The extended references of one hook call: the E-step's record (em_phase_reference.estep_reference: p_vl, its bound
    b_pvl, the floored s) and the smoother's w and bar on the operands p_vl * lweight with the bound b_pvl * lweight."""
    from em_phase_reference import estep_reference
    from oracle import em_numpy as em
    est = estep_reference(em.pdf_params(case["cnn"].copy()), case["v"], case["lp"], case["s"])
    lw = ld(case["lweight"])
    w, bar = smooth_reference(est["p_vl"] * lw[None, :], est["b_pvl"] * lw[None, :], case["lweight"], case["lsim"], case["bias"])
    return est, w, bar
