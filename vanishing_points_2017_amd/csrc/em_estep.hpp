// em_estep.hpp -- the E-step, with the panel geometry of the row-sliced smoother and the plan that chooses it: the E-step writes the
// operand panel that plan describes, so the three stay together.
// One part of em_device.hpp (the conventions, and why the unit is compiled with -ffp-contract=off, are there).
#ifndef VPK_EM_ESTEP_HPP_
#define VPK_EM_ESTEP_HPP_

#include "em_ctx.hpp"

namespace vpk {

// ---- geometry of the row-sliced smoother (smooth_rows) -----------------------------------------------------------
// The N rows of lsim are cut into EIGHT slices of jch = ceil(N / 8) consecutive rows (the summation order every stored
// result was produced with: per (column, VP) eight ascending fma chains, then ((((p0 + p1) + p2) + ...) + p7).  The
// operand panel w_[line][vp] is kept slice by slice, [slice][row in slice][W], with the slice stride padded to 16 mod 32
// doubles so that the two slices whose rows one ds_read_b64 touches (lanes 0-31: two rows of 16 lanes) lie in
// different halves of the 64 banks.
constexpr int RS_TT = 4;                               // VPs per reduction round (one output per lane and round)
constexpr int RS_RED_DOUBLES = RS_TT * 16 * 9;         // per wave: [vp][column][8 slices + 1 pad]
constexpr int RS_PANEL_FLAG = 0x100;                   // sh.ibuf[5] = RS_PANEL_FLAG + W: the E-step left this layout
VPK_DEV int rs_jchunk(int N) { return (N + 7) >> 3; }
VPK_DEV int rs_sstride(int jch, int W) { const int q = jch * W; return q + ((16 - q) & 31); }
VPK_DEV int rs_panel_doubles(int jch, int W) { return 8 * rs_sstride(jch, W) + 32; }   // + slack: lanes read 16 + i past a row
VPK_DEV int rs_row(int n, int jch, int S, int W) { const int sl = n / jch; return sl * S + (n - sl * jch) * W; }
// Which smoother the next smooth() takes for M hypotheses -- decided in ONE place because the E-step writes the panel in
// that smoother's layout.  0: none in LDS (wsrc in HBM), 1: smooth_full's [line][W], 2: smooth_rows' sliced layout.
// VPs per pass of smooth_rows when the whole panel does not fit: the widest multiple of 8 (<= 32) whose sliced panel and
// the reduction scratch fit the LDS budget; 0 = not even 8
VPK_DEV int rs_wfit(const EmCtx& c) {
    const int jch = rs_jchunk(c.N);
    for (int w = 32; w >= MT; w -= MT)
        if (rs_panel_doubles(jch, w) + 8 * RS_RED_DOUBLES <= c.wt_doubles) return w;
    return 0;
}
// Which smoother the next smooth() takes for M hypotheses -- decided in ONE place because the E-step writes the panel in
// that smoother's layout.  0: none in LDS (wsrc in HBM; smooth_full in passes or smooth_blocks), 1: smooth_full's
// [line][W], 2: smooth_rows' sliced layout, 3: wsrc in HBM, smooth_rows in passes of rs_wfit() VPs.
VPK_DEV int smooth_plan(const EmCtx& c, int M) {
    const int N = c.N;
    if (!c.prm.use_weights || M <= 0) return 0;
    const int Wp = ((M + MT - 1) / MT) * MT;
    const bool rows_ok = WAVE == 64 && nwaves() == 8 && c.smoother != 1;
    const int colw = N > WAVE ? 2 * WAVE : WAVE;                   // smooth_full's column groups: when they divide evenly
    const bool direct = (((N + colw - 1) / colw) % 8) == 0;        // among the waves it sums ALL rows in one chain
    if (M <= 32) {
        if (rows_ok && !direct && rs_panel_doubles(rs_jchunk(N), Wp) + 8 * RS_RED_DOUBLES <= c.wt_doubles) return 2;
        if ((long long)N * Wp <= c.wt_doubles) return 1;
    }
    // In passes: smooth_rows keeps smooth_full's eight-slice order, so it may stand in wherever smooth_full would run
    // (a panel of at least 8 VPs fits the OLD layout: wfit >= 8), never for smooth_blocks (one chain per column).
    if (rows_ok && !direct && (c.wt_doubles / N) / MT >= 1 && rs_wfit(c) >= MT) return 3;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// the E-step's distance, per measure
// ---------------------------------------------------------------------------------------------
// The per-pair value lvsq[n][m] per measure -- what differs between them; calc_plv, the p_l chain with its floor, the panel layouts
// and the lanes per line behind it do not see the measure.  estep_device.hpp's estep_lvsq<MEASURE>, restated operand for operand
// (that file restates this one; neither includes the other).  The EM runs the first two (vp_localisation.py:196-203; em_run asserts
// it); "area" is instantiated by the stand-alone merge_vps alone (vpset_device.hpp).
//   angle (:165-174):   the five rows line_geometry_setup<VPK_DIST_ANGLE> left in c.drow (midpoint, direction, its norm) against the
//                       VP projected to the image plane (sh.vx, sh.vy, written by the prior part below); a VP at infinity is a NaN column.
//   dotprod (:151-152): three rows, the normalised line c.l, against the VP as given in X (no division by v2: finite at infinity).
//   area (:187-207):    five rows (midpoint, first end point, c = |midpoint - second end point|) against sh.vx, sh.vy; the VP's part of
//                       vl = np.cross(v_, lmh) / |vl[0:2]| (estep_device.hpp's estep_vp<VPK_DIST_AREA>) is evaluated per pair from those
//                       two, the same expressions on the same operands: Shared keeps its size.  A negative radicand is a NaN.
struct EstepLine { double g0, g1, g2, g3, g4; };
template <int MEASURE> VPK_DEV EstepLine estep_line(const EmCtx& c, int n) {
    EstepLine g;
    g.g0 = c.drow[n]; g.g1 = c.drow[(size_t)c.ldn + n]; g.g2 = c.drow[2 * (size_t)c.ldn + n];
    if (MEASURE != VPK_DIST_DOTPROD) { g.g3 = c.drow[3 * (size_t)c.ldn + n]; g.g4 = c.drow[4 * (size_t)c.ldn + n]; }
    else { g.g3 = 0.0; g.g4 = 0.0; }
    return g;
}
template <int MEASURE> VPK_DEV double estep_pair(const EstepLine& g, const Shared& sh, const double* X, int m) {
    if (MEASURE == VPK_DIST_ANGLE) {
        const double v1x = g.g0 - sh.vx[m], v1y = g.g1 - sh.vy[m];
        const double n1 = norm2(v1x, v1y);
        const double cc = 1 - fabs(dot2(v1x, v1y, g.g2, g.g3) / (n1 * g.g4));
        return cc * cc;                                      // :174
    } else if (MEASURE == VPK_DIST_DOTPROD) {
        const double lv = (g.g0 * X[3 * m] + g.g1 * X[3 * m + 1]) + g.g2 * X[3 * m + 2];   // :151
        return lv * lv;                                      // :152
    } else {
        const double vx = sh.vx[m], vy = sh.vy[m];           // :187-188
        const double nrm = norm2(vy, -vx);                   // :201
        const double vl2 = (vx * g.g1 - vy * g.g0) / nrm;    // :200-201
        const double b = fabs(((vy / nrm) * g.g2 + (-vx / nrm) * g.g3) + vl2);   // :203
        const double a = sqrt(g.g4 * g.g4 - b * b);          // :205
        const double t = (a * (b * b)) / g.g4;
        return t * t;                                        // :207
    }
}

// ---------------------------------------------------------------------------------------------
// the line part without the responsibilities that are zero (the panel forms: plan 1 and plan 2)
// ---------------------------------------------------------------------------------------------
// Four in five of the terms p_lv p_v = exp(a) k2 pv, a = -(lvsq / 2s), are +0.0 because exp underflows (em_smooth.hpp counts the
// same zeros among the smoother's operands), and so are their responsibilities term / p_l: two divisions and an exp per pair, some 70
// instructions, that end in a value known beforehand.  The lanes of a wave run in lockstep and nearly every VP has SOME line of the
// wave that needs its exp, so a test inside the dense VP loop saves nothing.  The panel forms therefore run three passes:
//   A  (dense)   lvsq for every VP of the lane's range, parked in the line's panel slot; a VP is KEPT -- a bit of a 64-bit mask
//                (MAXM = 64) -- unless lvsq > (2 s) ESTEP_UNDERFLOW_BOUND holds, which implies a < -746.0 (below) and costs a
//                product where a costs a division.  A NaN lvsq is kept, and so is the narrow band in which a < -746.0 holds and
//                the cheaper test does not see it: those take the dense form's own arithmetic in pass B;
//   B  (sparse)  the kept VPs only, in ascending order: a and the term, with exp_underflow's value and the dense form's grouping,
//                parked in the slot and added to p_l in that order.  The loop lasts as long as the lane of the wave with most kept
//                VPs;
//   C            term / p_l and its product with lweight for the kept VPs; for all others 0.0 / p_l and (0.0 / p_l) * lweight,
//                evaluated once per line.
// SAME BITS, BY CONSTRUCTION.  The dense form's term of a VP that is not kept is (0.0 * k2[m]) * pv[m], exp_underflow returning
// 0.0 below -746.  That is +0.0 exactly when k2[m] and pv[m] are finite and of equal sign (estep_zero_safe: one wave-uniform mask
// per call); a VP outside that mask is kept by EVERY lane and takes the dense form's arithmetic, whatever its lvsq.  Then
//   * p_l: the dense chain starts at +0.0 and a sum of two doubles is -0.0 only if both are, so the running sum is never -0.0, and
//     x + (+0.0) = x for every other x, NaN and infinities included: leaving the +0.0 terms out leaves every partial sum as it was,
//     also the sum a lane takes over from its neighbour (T > 1).
//   * p_vl and the panel: the dense form divides the parked +0.0 by p_l and multiplies by lweight; pass C evaluates that very
//     expression on those very operands, once.
// The cases that would break it if handled carelessly:
//   * a NaN column (a VP at infinity under "angle": vx, vy are inf or NaN, lvsq NaN): lvsq > bound is false, kept.
//   * a NaN or infinite pv (a VP whose angles are NaN, an overflowing mixture): 0.0 * pv is NaN, not +0.0 -- the VP is outside
//     the mask, all its terms are evaluated and p_l becomes the NaN the dense form makes.
//   * s at its 1e-200 floor: k2 ~ 4e99 stays finite and the bound, 1.5e-197, is a normal number: every lvsq above it is left out,
//     lvsq = 0 or NaN is kept; a huge s (max_stdd and beyond) keeps everything, and so does an infinite one (bound inf, k2 = +0.0).
//   * a line all of whose terms underflow: nothing is kept, p_l stays +0.0 and is floored to 1e-12, and every entry of the line is
//     0.0 / 1e-12 = +0.0 -- what pass C stores.  A NaN p_l (it passes the floor) makes 0.0 / p_l NaN in both forms.
//   * -0.0: a negative pv (or k2) with the other positive makes the dense term -0.0, whose quotient is -0.0, not pass C's +0.0:
//     hence the sign test in the mask.  A kept term that comes out as -0.0 is added and divided as before.
// lvsq > (2 s) * this  =>  -(lvsq / (2 s)) < -746.0.  The constant is 746 (1 + 2^-40) and 2 s is exact, so the rounded product lies
// above 746 (2 s) by more than 2^-41 of it; then the true quotient lies above 746 (1 + 2^-41) and the rounded quotient (rounding is
// monotone, and doubles between 746 and that value exist) above 746.  s >= 1e-200: no subnormal product; an overflowing one keeps.
constexpr double ESTEP_UNDERFLOW_BOUND = 746.0 * (1.0 + 0x1p-40);
typedef unsigned long long vpmask_t;
VPK_DEV int lowest_vp(vpmask_t r) { return __builtin_ctzll(r); }
VPK_DEV bool estep_zero_safe(double k2, double pv) {
    return fabs(k2) <= 1.7976931348623157e308 && fabs(pv) <= 1.7976931348623157e308 &&
           (__double_as_longlong(k2) < 0) == (__double_as_longlong(pv) < 0);
}
// bit m: VP m's underflowed term is +0.0.  Called by every lane of the workgroup; the result is wave-uniform.
VPK_DEV vpmask_t estep_zero_safe_mask(const Shared& sh, int M) {
    if (WAVE == MAXM) {                                      // lane m tests VP m
        const int m = lane() < M ? lane() : 0;
        return wave_ballot(lane() < M && estep_zero_safe(sh.k2[m], sh.pv[m]));
    }
    vpmask_t r = 0;
    for (int m = 0; m < M; ++m) r |= (vpmask_t)estep_zero_safe(sh.k2[m], sh.pv[m]) << m;
    return r;
}
// exp_underflow's value for every x, without its branch (two of these run side by side)
VPK_DEV double exp_underflow_select(double x) {
    const double e = exp(x);
    return x < -746.0 ? 0.0 : e;
}
// pass A over the VPs [m_lo, m_hi) of one line: lvsq to lvq and to the panel slot; force: the VPs every lane keeps.  Returns the kept VPs.
template <int MEASURE>
VPK_DEV vpmask_t estep_keep(const EstepLine& g, const Shared& sh, const double* X, int m_lo, int m_hi, vpmask_t force,
                            gdp lvq, int ldn, double* wl) {
    constexpr int EU = 4;                                    // four sqrt / div chains side by side, as in the dense form
    const int cnt = m_hi - m_lo;
    const vpmask_t range = cnt <= 0 ? 0ull : ((cnt >= 64 ? ~0ull : (1ull << cnt) - 1ull) << m_lo);
    vpmask_t keep = force & range;
    int m = m_lo;
    for (; m + EU <= m_hi; m += EU) {
        double lv[EU], bound[EU];
#pragma unroll
        for (int u = 0; u < EU; ++u) lv[u] = estep_pair<MEASURE>(g, sh, X, m + u);
#pragma unroll
        for (int u = 0; u < EU; ++u) bound[u] = (2 * sh.s[m + u]) * ESTEP_UNDERFLOW_BOUND;
#pragma unroll
        for (int u = 0; u < EU; ++u) {
            lvq[(size_t)(m + u) * ldn] = lv[u];
            wl[m + u] = lv[u];
            keep |= (vpmask_t)(!(lv[u] > bound[u])) << (m + u);
        }
    }
    for (; m < m_hi; ++m) {
        const double lv1 = estep_pair<MEASURE>(g, sh, X, m);
        lvq[(size_t)m * ldn] = lv1;
        wl[m] = lv1;
        keep |= (vpmask_t)(!(lv1 > (2 * sh.s[m]) * ESTEP_UNDERFLOW_BOUND)) << m;
    }
    return keep;
}
// pass B: the kept terms in ascending VP order, two at a time; SUM: added to pl in that order.  Returns pl.
template <bool SUM> VPK_DEV double estep_terms(vpmask_t keep, const Shared& sh, double* wl, double pl) {
    vpmask_t r = keep;
    while (r != 0) {
        const int m0 = lowest_vp(r);
        r &= r - 1;
        const bool two = r != 0;
        const int m1 = two ? lowest_vp(r) : m0;
        r &= r - 1;                                          // (0 stays 0)
        const double a0 = -(wl[m0] / (2 * sh.s[m0])), a1 = -(wl[m1] / (2 * sh.s[m1]));   // calc_plv :137
        const double t0 = (exp_underflow_select(a0) * sh.k2[m0]) * sh.pv[m0];   // calc_plv :137-145
        const double t1 = (exp_underflow_select(a1) * sh.k2[m1]) * sh.pv[m1];
        wl[m0] = t0;
        if (SUM) pl += t0;                                   // p_l = dot(p_lv, p_v) :116, in VP order
        if (two) {
            wl[m1] = t1;
            if (SUM) pl += t1;
        }
    }
    return pl;
}
// pass C over the VPs [m_lo, m_hi) of one line, pl floored
VPK_DEV void estep_posteriors(vpmask_t keep, int m_lo, int m_hi, double pl, double lw, gdp pvq, int ldn, double* wl) {
    const double z = 0.0 / pl, zl = z * lw;                  // calc_pvl :128 and weight_matrix :519 of a term that is +0.0
    for (int m = m_lo; m < m_hi; ++m)
        if (!((keep >> m) & 1)) {
            pvq[(size_t)m * ldn] = z;
            wl[m] = zl;
        }
    vpmask_t r = keep;
    while (r != 0) {
        const int m0 = lowest_vp(r);
        r &= r - 1;
        const bool two = r != 0;
        const int m1 = two ? lowest_vp(r) : m0;
        r &= r - 1;
        const double q0 = wl[m0] / pl, q1 = wl[m1] / pl;     // calc_pvl :128
        pvq[(size_t)m0 * ldn] = q0;
        wl[m0] = q0 * lw;                                    // weight_matrix :519
        if (two) {
            pvq[(size_t)m1 * ldn] = q1;
            wl[m1] = q1 * lw;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// E-step: calc_probabilities (probability_functions.py:99-147), the measure a template parameter
// ---------------------------------------------------------------------------------------------
// X points at sh.cur or sh.nxt.  Writes lvsq[m][n], pvl[m][n], wsrc[n][m]; floors sh.s (:139).
// (Round 6, measured: the body inlined into em_run's main loop -- to save the callee-saved register traffic of one call per iteration,
//  which did pay for the smoother's thin wrappers -- makes the E-step 2.5 x SLOWER, 51 -> 130 ms of workgroup time per YUD batch: inside
//  em_run's register allocation the line loop spills.  The phases stay functions of their own.)
template <int MEASURE = VPK_DIST_ANGLE>
VPK_DEVFN void estep(EmCtx& c, const double* X) {
    Shared& sh = SH();
    const int M = sh.M, N = c.N;
    const double kk = -0.5 / (sh.sigma_prior * sh.sigma_prior);
    long long tq_ = clock_ticks();
    // prior p(v): a group of VPG lanes per VP (four VPs per wave: the asin/cos chains of four VPs run in one
    // wave's lanes), lanes over mixture components (calc_angles :252-259, calc_pdf :8-40)
    {
        constexpr int G = VPG;
        const int gl = lane() % G;
        const int per_round = nwaves() * (WAVE / G);
        for (int m = wave_id() * (WAVE / G) + lane() / G; m < M; m += per_round) {
            double x0 = X[3 * m], x1 = X[3 * m + 1], x2 = X[3 * m + 2];
            double alpha, beta;
            vp_angles(x0, x1, alpha, beta);
            double acc = 0.0;
            for (int q = gl; q < sh.ncomp; q += G) {
                acc += mixture_term(alpha, beta, sh.pma[q], sh.pmb[q], kk) * sh.pw[q];
            }
            acc = group_sum<G>(acc);
            if (gl == 0) {
                sh.pv[m] = acc;
                if (MEASURE != VPK_DIST_DOTPROD) {
                    sh.vx[m] = x0 / x2;                      // calc_lvsq_angle :165-166, calc_lvsq_area :187-188
                    sh.vy[m] = x1 / x2;
                }
                double sm = sh.s[m];
                sm = sm > 1e-200 ? sm : 1e-200;              // calc_plv :139 (in place)
                sh.s[m] = sm;
                sh.k2[m] = 1.0 / sqrt(2 * PI_D * sm);        // :145
            }
        }
    }
    block_sync();
    if (tid() == 0) sh.dbuf[14] += lap(tq_);
    // When the smoother's whole operand panel fits in LDS the weights go there directly ([line][vp],
    // Wp = M rounded to the VP tile) as well as to HBM, and smooth_full skips its staging pass.
    const int Wp = ((M + MT - 1) / MT) * MT;
    const int plan = smooth_plan(c, M);                      // 1: [line][Wp] for smooth_full, 2: slice by slice for smooth_rows
    const bool panel = plan == 1 || plan == 2;
    const int rs_jch = rs_jchunk(N), rs_S = rs_sstride(rs_jch, Wp);
    double* wt = WT();
    // one thread per line; the VP loop is unrolled four deep with the four sqrt/div/exp chains written
    // side by side (independent until the ordered sum), because a lone wave per SIMD is bound by the
    // latency of that dependent chain, not by issue
    constexpr int EU = 4;
    // LANES PER LINE (round 6).  One thread per line leaves 512 - N threads idle and the busy ones with M dependent sqrt / div / exp
    // chains each: at the YUD shape (N ~ 250, M ~ 22) the line part took as long as the smoother's row loops.  When the panel is in
    // LDS and T N <= 512, T = 2, 4 or 8 ADJACENT lanes share a line, each a contiguous run of ceil(M / T) VPs.  Every (line, VP) value
    // is the same expression as below; p_l (:116) is still ONE chain over the VPs in ascending order -- lane h takes the running sum
    // from lane h - 1 and continues it over its own terms, re-read from the line's panel row -- so every output has the same bits.
    // THE ZERO RESPONSIBILITIES LEFT OUT.  With the panel in LDS the line part runs as three passes, the exp and the division to p_vl
    // only for the VPs whose term does not underflow (see above); the dense loop below serves the plans without a panel and, under
    // vpk_em_set_smoother(1), every plan: the form the three passes are held to, bit for bit.
    const bool sparse = panel && c.smoother != 1;
    const vpmask_t force = ~estep_zero_safe_mask(sh, M);     // the VPs every lane keeps (wave-uniform: scalar registers)
    int T = 1;
    if (sparse && WAVE == 64)                                // (vpk_em_set_smoother(1): the forms of the earlier rounds, for the bit-equality test)
        while (T < 8 && 2 * T * N <= nthreads()) T *= 2;
    if (T > 1) {
        const int n_ = tid() / T, h = tid() - n_ * T;
        const bool on = n_ < N;
        const int n = on ? n_ : N - 1;
        const int Mh = (M + T - 1) / T;
        const int m_lo = on ? (h * Mh < M ? h * Mh : M) : 0, m_hi = on ? (m_lo + Mh < M ? m_lo + Mh : M) : 0;
        const EstepLine g = estep_line<MEASURE>(c, n);
        const double lw = c.lweight[n];
        gdp lvq = c.lvsq + n, pvq = c.pvl + n;
        double* wl = wt + (plan == 2 ? (size_t)rs_row(n, rs_jch, rs_S, Wp) : (size_t)n * Wp);
        const vpmask_t keep = estep_keep<MEASURE>(g, sh, X, m_lo, m_hi, force, lvq, c.ldn, wl);   // pass A
        estep_terms<false>(keep, sh, wl, 0.0);               // pass B: the terms, parked in the line's panel row
        double pl = 0.0;                                     // p_l = dot(p_lv, p_v) :116, in VP order, handed from lane to lane
        for (int hh = 0; hh < T; ++hh) {
            const double prev = wave_bcast(pl, (lane() + WAVE - 1) & (WAVE - 1));
            if (h == hh) {
                if (hh > 0) pl = prev;
                for (vpmask_t r = keep; r != 0; r &= r - 1) pl += wl[lowest_vp(r)];   // (the terms left out are +0.0)
            }
        }
        pl = wave_bcast(pl, lane() | (T - 1));               // the line's last lane holds the whole sum
        pl = (pl > 1e-12 || is_nan(pl)) ? pl : 1e-12;        // :117
        estep_posteriors(keep, m_lo, m_hi, pl, lw, pvq, c.ldn, wl);   // pass C
        if (on && h == T - 1)
            for (int m = M; m < Wp; ++m) wl[m] = 0.0;        // padding of the last VP tile
    } else if (sparse)
    for (int n = tid(); n < N; n += nthreads()) {            // one thread per line, the three passes
        const EstepLine g = estep_line<MEASURE>(c, n);
        gdp lvq = c.lvsq + n, pvq = c.pvl + n;
        double* wl = wt + (plan == 2 ? (size_t)rs_row(n, rs_jch, rs_S, Wp) : (size_t)n * Wp);
        const vpmask_t keep = estep_keep<MEASURE>(g, sh, X, 0, M, force, lvq, c.ldn, wl);
        double pl = estep_terms<true>(keep, sh, wl, 0.0);    // p_l = dot(p_lv, p_v) :116, in VP order
        pl = (pl > 1e-12 || is_nan(pl)) ? pl : 1e-12;        // :117
        estep_posteriors(keep, 0, M, pl, c.lweight[n], pvq, c.ldn, wl);
        for (int m = M; m < Wp; ++m) wl[m] = 0.0;            // padding of the last VP tile
    } else
    for (int n = tid(); n < N; n += nthreads()) {
        const EstepLine g = estep_line<MEASURE>(c, n);
        gdp lvq = c.lvsq + n, pvq = c.pvl + n;
        double* wl = wt + (plan == 2 ? (size_t)rs_row(n, rs_jch, rs_S, Wp) : (size_t)n * Wp);   // this line's panel row; parks p_lv p_v until p_l is known
        double pl = 0.0;
        int m = 0;
        for (; m + EU <= M; m += EU) {
            double lv[EU], tt[EU];
#pragma unroll
            for (int u = 0; u < EU; ++u) lv[u] = estep_pair<MEASURE>(g, sh, X, m + u);
#pragma unroll
            for (int u = 0; u < EU; ++u)
                tt[u] = (exp_underflow(-(lv[u] / (2 * sh.s[m + u]))) * sh.k2[m + u]) * sh.pv[m + u];   // calc_plv :137-145
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                lvq[(size_t)(m + u) * c.ldn] = lv[u];
                if (panel) wl[m + u] = tt[u]; else pvq[(size_t)(m + u) * c.ldn] = tt[u];
                pl += tt[u];                                 // p_l = dot(p_lv, p_v) :116, in VP order
            }
        }
        for (; m < M; ++m) {
            const double lv1 = estep_pair<MEASURE>(g, sh, X, m);
            lvq[(size_t)m * c.ldn] = lv1;
            const double t1 = (exp_underflow(-(lv1 / (2 * sh.s[m]))) * sh.k2[m]) * sh.pv[m];
            if (panel) wl[m] = t1; else pvq[(size_t)m * c.ldn] = t1;
            pl += t1;
        }
        pl = (pl > 1e-12 || is_nan(pl)) ? pl : 1e-12;        // :117
        const double lw = c.lweight[n];
        gdp ws = c.wsrc + (size_t)n * c.mcap;
        m = 0;
        for (; m + EU <= M; m += EU) {
            double q[EU];
#pragma unroll
            for (int u = 0; u < EU; ++u) q[u] = panel ? wl[m + u] : pvq[(size_t)(m + u) * c.ldn];
#pragma unroll
            for (int u = 0; u < EU; ++u) q[u] = q[u] / pl;   // calc_pvl :128
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                pvq[(size_t)(m + u) * c.ldn] = q[u];
                if (panel) wl[m + u] = q[u] * lw;            // weight_matrix :519 (the HBM copy has no reader when the
                else ws[m + u] = q[u] * lw;                  //   smoother takes the whole panel from LDS in one pass)
            }
        }
        for (; m < M; ++m) {
            const double q1 = (panel ? wl[m] : pvq[(size_t)m * c.ldn]) / pl;
            pvq[(size_t)m * c.ldn] = q1;
            if (panel) wl[m] = q1 * lw; else ws[m] = q1 * lw;
        }
        for (m = M; m < Wp; ++m) {                           // padding of the last VP tile
            if (panel) wl[m] = 0.0; else ws[m] = 0.0;
        }
    }
    if (plan == 2)                                           // zero operand rows where a short or empty slice has no line
        for (int p = N * Wp + tid(); p < 8 * rs_jch * Wp; p += nthreads()) {
            const int j = p / Wp;
            wt[rs_row(j, rs_jch, rs_S, Wp) + (p - j * Wp)] = 0.0;
        }
    if (tid() == 0) sh.dbuf[15] += lap(tq_);
    if (tid() == 0) sh.ibuf[5] = plan == 2 ? RS_PANEL_FLAG + Wp : (plan == 1 ? Wp : 0);   // consumed (and cleared) by smooth()
    block_sync();
}

}  // namespace vpk
#endif
