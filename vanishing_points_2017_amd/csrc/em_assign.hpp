// em_assign.hpp -- line -> VP association, line counts per VP and the compaction of the VP set.
// One part of em_device.hpp (the conventions, and why the unit is compiled with -ffp-contract=off, are there).
#ifndef VPK_EM_ASSIGN_HPP_
#define VPK_EM_ASSIGN_HPP_

#include "em_ctx.hpp"

namespace vpk {

// ---------------------------------------------------------------------------------------------
// line -> VP association and counts: calc_vp_line_counts (vp_localisation.py:482-512)
// ---------------------------------------------------------------------------------------------
// np.argmax over VPs (first maximum; a NaN counts as the maximum).  hard = apply the outlier test.
// The outlier test's distance (:495-498): "angle" calc_lvsq_single = the E-step's lvsq of that pair; "dotprod" |vp . l| (:496), taken as
// sqrt(lvsq) of the E-step that has just run on the same VPs -- within an ulp of the reference's own dot product, so the stored
// reference results are recorded only where no line comes within 1e-9 relative of its threshold (scripts/make_em_dotprod_goldens.py).
template <int MEASURE = VPK_DIST_ANGLE>
VPK_DEVFN void assign_lines(EmCtx& c, bool hard) {
    Shared& sh = SH();
    const int M = sh.M, N = c.N;
    for (int n = tid(); n < N; n += nthreads()) {
        int best = 0;
        double bv = c.w[n];
        for (int m = 1; m < M; ++m) {
            double v = c.w[(size_t)m * c.ldn + n];
            if (!is_nan(bv) && (v > bv || is_nan(v))) { bv = v; best = m; }
        }
        if (hard && M > 0) {
            double dist = c.lvsq[(size_t)best * c.ldn + n];   // == calc_lvsq_single on the same VP slice
            if (MEASURE == VPK_DIST_DOTPROD) dist = sqrt(dist);
            if (dist > c.prm.outlier_thresh * sqrt(sh.s[best]))
                best = -1;                                    // :504
            else if (c.lweight[n] == 0)
                best = -1;                                    // :506
        }
        c.assoc[n] = best;
    }
    block_sync();
}
VPK_DEVFN void count_lines(EmCtx& c) {
    Shared& sh = SH();
    const int M = sh.M, N = c.N;
    for (int m = wave_id(); m < M; m += nwaves()) {
        int cnt = 0;
        double cw = 0.0;
        for (int n = lane(); n < N; n += WAVE)
            if (c.assoc[n] == m) { ++cnt; cw += c.lweight[n]; }
        cnt = wave_sum_int(cnt);
        cw = wave_sum(cw);
        if (lane() == 0) { sh.cnt[m] = (double)cnt; sh.cntw[m] = cw; }
    }
    block_sync();
}

// remove the VPs flagged in sh.removed from cur / nxt / s (np.delete along the VP axis)
VPK_DEV void compact_vps(EmCtx& c) {
    Shared& sh = SH();
    static_assert(MAXM <= 64, "compact_vps: one lane per hypothesis");
    if (WAVE == 64 && c.smoother != 1) {
        // MAXM = 64 hypotheses = the lanes of one wave: lane m keeps its VP's values in registers, a ballot of the survivors gives
        // every survivor its new index (popcount of the survivors below it), and the common case -- nothing removed, every
        // iteration of a settled image -- writes nothing at all.  (One thread walking the list cost ~2 us per call.)
        if (wave_id() == 0) {
            const int M = sh.M, m = lane();
            const bool keep = m < M && !sh.removed[m];
            const unsigned long long km = wave_ballot(keep);
            const int kept = popcount64(km);
            if (kept != M) {
                double v[7];
                if (keep) {
                    for (int d = 0; d < 3; ++d) { v[d] = sh.cur[3 * m + d]; v[3 + d] = sh.nxt[3 * m + d]; }
                    v[6] = sh.s[m];
                }
                wave_lds_order();
                const int k = popcount64(km & lanes_below());
                if (keep && k != m) {
                    for (int d = 0; d < 3; ++d) { sh.cur[3 * k + d] = v[d]; sh.nxt[3 * k + d] = v[3 + d]; }
                    sh.s[k] = v[6];
                }
                if (m == 0) sh.M = kept;
            }
        }
        block_sync();
        return;
    }
    if (tid() == 0) {
        int k = 0;
        for (int m = 0; m < sh.M; ++m) {
            if (sh.removed[m]) continue;
            if (k != m) {
                for (int d = 0; d < 3; ++d) {
                    sh.cur[3 * k + d] = sh.cur[3 * m + d];
                    sh.nxt[3 * k + d] = sh.nxt[3 * m + d];
                }
                sh.s[k] = sh.s[m];
            }
            ++k;
        }
        sh.M = k;
    }
    block_sync();
}

}  // namespace vpk
#endif
