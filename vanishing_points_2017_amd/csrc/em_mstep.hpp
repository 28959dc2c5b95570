// em_mstep.hpp -- the M-step and the largest per-VP error.
// One part of em_device.hpp (the conventions, and why the unit is compiled with -ffp-contract=off, are there).
#ifndef VPK_EM_MSTEP_HPP_
#define VPK_EM_MSTEP_HPP_

#include "em_ctx.hpp"
#include "em_linalg.hpp"

namespace vpk {

// ---------------------------------------------------------------------------------------------
// M-step: calc_new_vanishing_point (vp_localisation.py:453-479) + variance (:301-307)
// ---------------------------------------------------------------------------------------------
// One group of VPG lanes per VP (four VPs per wave: the serial 3x3 eigen-solves of four VPs then run in
// the lanes of one wave instead of four waves' worth of rounds).  mode 0: soft (all lines, weights w[m]); mode 1: hard (lines with
// assoc == m, :353-392).  On return sh.removed[] / sh.err[] are set; nxt and s updated.
// LB = lines whose loads are in flight per lane (group_null_vector).  Four at the sizes whose arrays live in L2 (measured: eight is slower
// there); large images (N >= 512: ECD / HLW / the stress shape) walk N / 16 >= 32 lines per lane through arrays that come from HBM beside
// 255 other workgroups' lsim streams -- there the walk is a chain of memory round trips (73 us per M-step at the stress shape, 42 alone)
// and twice the loads in flight halve it.  Same lines in the same order per lane: same bits.
// (Round 6 also measured a whole WAVE per hypothesis for large images with at most eight hypotheses -- another summation order, so other
//  bits; every golden and all four config tables stayed green --: the stress shape's M-step 61 -> 39 us per call, and the launch 60.6 ->
//  59.0 ms: the time moves into the smoother, whose stream then shares the HBM with more workgroups.  Not worth new bits.)
template <int LB>
VPK_DEVFN void mstep_lb(EmCtx& c, int mode, double max_stdd) {
    Shared& sh = SH();
    const int M = sh.M, N = c.N;
    constexpr int G = VPG;
    const int gl = lane() % G;
    const int per_round = nwaves() * (WAVE / G);
    for (int m = wave_id() * (WAVE / G) + lane() / G; m < M; m += per_round) {
        cgdp wm = c.w + (size_t)m * c.ldn;
        double wmax = -1e300;
        int nsel = 0, selidx = -1;
        double sv = 0, sp = 0;
        cgdp lvs = c.lvsq + (size_t)m * c.ldn;
        cgdp pvl = c.pvl + (size_t)m * c.ldn;
        for (int n0 = gl; n0 < N; n0 += LB * G) {
            double pq[LB], lq[LB], wq[LB];
            int aq[LB];
#pragma unroll
            for (int u = 0; u < LB; ++u) {
                const int n = n0 + u * G;
                const int nc = n < N ? n : 0;
                pq[u] = pvl[nc]; lq[u] = lvs[nc]; wq[u] = wm[nc];
                aq[u] = mode == 1 ? c.assoc[nc] : m;
            }
#pragma unroll
            for (int u = 0; u < LB; ++u) {
                const int n = n0 + u * G;
                if (n >= N) break;
                sv += lq[u] * pq[u];                          // :303 (all lines, also in hard mode :374)
                sp += pq[u];
                if (mode == 1 && aq[u] != m) continue;
                wmax = nanmax(wmax, wq[u]);
                ++nsel;
                selidx = n;
            }
        }
        wmax = group_max<G>(wmax);
        nsel = group_sum_int<G>(nsel);
        selidx = group_max_int<G>(selidx);
        sv = group_sum<G>(sv);
        sp = group_sum<G>(sp);
        if (mode == 1 && nsel == 0) {                         // :355-356 `continue`
            if (gl == 0) { sh.removed[m] = 0; sh.err[m] = -1.0; }
            continue;
        }
        bool valid = nsel > 0 && (wmax > 0 || wmax < 0);      // :456-460; NaN -> LinAlgError -> None
        double vp[3] = {0, 0, 0};
        if (valid && nsel > 1) {
            const VPK_GLOBAL int* assoc = c.assoc;
            // row weight w / max w (:462; hard mode: :358 then / 1 at :462)
            group_null_vector<G, LB>(c.l, N, [=](int n) { return (mode == 1 && assoc[n] != m) ? 0.0 : wm[n] / wmax; }, vp);
        }
        if (gl == 0) {
            int rem = 0;
            double err = -1.0;
            if (!valid) {
                rem = 1;                                      // newVP is None (:294-296)
            } else {
                if (nsel == 1) {                              // one row: LAPACK's reflector decides
                    cgdp ln = c.l + 3 * (size_t)selidx;
                    lapack_null_1row(ln[0], ln[1], ln[2], vp);    // the row is (w/max w) * l = 1 * l
                    double nr = norm3(vp[0], vp[1], vp[2]);
                    vp[0] /= nr; vp[1] /= nr; vp[2] /= nr;    // :472
                }
                double sg = sign_np(vp[2]);                   // :474
                vp[0] *= sg; vp[1] *= sg; vp[2] *= sg;
                sh.nxt[3 * m] = vp[0]; sh.nxt[3 * m + 1] = vp[1]; sh.nxt[3 * m + 2] = vp[2];
                double sm = exp(log(sv) - log(sp));           // :303-304
                sm = (sm < max_stdd || is_nan(sm)) ? sm : max_stdd;          // :306 np.minimum
                if (mode == 0)
                    sm = (sm > c.prm.s_thresh || is_nan(sm)) ? sm : c.prm.s_thresh;   // :307
                sh.s[m] = sm;
                if (is_nan(sm) || (mode == 1 && sm < c.prm.s_thresh)) {
                    rem = 1;                                  // :309-310 / :379-380
                } else {
                    double d = fabs(dot3(sh.cur[3 * m], sh.cur[3 * m + 1], sh.cur[3 * m + 2], vp[0], vp[1], vp[2]));
                    err = acos(d < 1.0 ? d : 1.0);            // :312
                    if (err > 1.5) rem = 1;                   // :316-317
                }
            }
            sh.removed[m] = rem;
            sh.err[m] = err;
        }
    }
    block_sync();
}

VPK_DEV void mstep(EmCtx& c, int mode, double max_stdd) {
    if (c.N >= 512 && c.smoother != 1) mstep_lb<8>(c, mode, max_stdd); else mstep_lb<4>(c, mode, max_stdd);
}

// max over the per-VP errors with np.maximum semantics (NaN sticks); VPs without an error are -1
VPK_DEV double max_err_of(const Shared& sh, int M) {
    double mx = 0.0;
    for (int m = 0; m < M; ++m) {
        double e = sh.err[m];
        if (e == -1.0) continue;
        mx = (is_nan(mx) || is_nan(e)) ? (is_nan(mx) ? mx : e) : (e > mx ? e : mx);
    }
    return mx;
}

}  // namespace vpk
#endif
