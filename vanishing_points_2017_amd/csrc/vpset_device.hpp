// vpset_device.hpp -- VP set maintenance outside the EM: calc_vp_line_counts (vp_localisation.py:482-512),
// split_best_vp (:527-630) and merge_vps (:633-684) on a caller-supplied VP set, one workgroup per image.  The phases are
// the EM workgroup's own device functions (em_assign.hpp: count_lines, compact_vps; em_vpset.hpp: split_vp with cluster2 /
// cluster2_lds, merge_vps with em_estep.hpp's estep, em_smooth.hpp's smooth and em_linalg.hpp's wave_null_vector); this header
// binds an EmCtx and the Shared block to the caller's arrays instead of running the EM's set-up, and adds the one step
// the EM never needs: the association from a caller's vp_assoc (:486, :494) tested against the caller's own s.
#ifndef VPK_VPSET_DEVICE_HPP_
#define VPK_VPSET_DEVICE_HPP_

#include "em_device.hpp"

namespace vpk {

typedef const VPK_GLOBAL long long* cgllp;
typedef VPK_GLOBAL long long* gllp;

constexpr int VPSET_COUNTS = 0, VPSET_SPLIT = 1, VPSET_MERGE = 2;

// Image b of the batch: lines [line_off[b], line_off[b + 1]), VPs [vp_off[b], vp_off[b + 1]), its (M x N) matrix at
// element mat_off[b], its workspace at double ws_off[b].  active[q] = the q-th image that has lines and VPs: the grid.
struct VpsetArgs {
    int op;
    cgllp line_off, vp_off, mat_off, ws_off, active;
    cgdp lp, l, v, s, w, lweight, langle;
    cgllp assoc_in;       // counts: NULL = argmax of the metric (:487)
    double thresh;        // counts: thresh (:504); split: min_diff (:614)
    gdp ws;
    int wt_doubles;
    // counts
    gdp counts, counts_w;
    gllp assoc_out;
    // split: image b's rows start at vp_off[b] + b (M_b + 1 rows each)
    gdp v_out, s_out;
    gip m_out, split_out, labels_out;
    VPK_GLOBAL unsigned* flags_out;
    // merge: one EM slot per image (L is sized for the batch's largest image); mat_off = the image's N x N lsim; outputs at
    // vp_off[b] (M_b rows each)
    EmLayout L;
    cgdp lsim;
    const VPK_GLOBAL float* prior_w;   // batch x 400
    double prior_sigma, wbias, max_stdd;
    gip keep_out;
};

// The distance of the outlier test (:495-500) for one (VP, line) pair, on the caller's v, lp and l as they stand: the
// reference normalises none of them here.
//   angle    calc_lvsq_single (probability_functions.py:212-224): the E-step's lvsq of the pair
//   dotprod  |vp[m] . l[n]| (:496), grouped as em_estep.hpp's estep_pair groups it; finite for a VP at infinity
//   area     calc_lvsq_area_single (probability_functions.py:227-249): estep_device.hpp's estep_line / estep_vp /
//            estep_lvsq<VPK_DIST_AREA> of the pair, restated operand for operand -- the E-step's lvsq again.  NaN where
//            c^2 - b^2 < 0 (:245) and, as under "angle", for a VP with v[2] == 0.
template <int MEASURE> VPK_DEV double vpset_dist(cgdp v, cgdp q, cgdp hl) {
    if (MEASURE == VPK_DIST_DOTPROD) return fabs((hl[0] * v[0] + hl[1] * v[1]) + hl[2] * v[2]);
    const double vx = v[0] / v[2], vy = v[1] / v[2];
    const double mx = 0.5 * (q[0] + q[2]), my = 0.5 * (q[1] + q[3]);
    if (MEASURE == VPK_DIST_ANGLE) {
        const double v1x = mx - vx, v1y = my - vy;
        const double v2x = q[0] - q[2], v2y = q[1] - q[3];
        const double cc = 1 - fabs(dot2(v1x, v1y, v2x, v2y) / (norm2(v1x, v1y) * norm2(v2x, v2y)));
        return cc * cc;
    }
    const double nrm = norm2(vy, -vx);                        // :241
    const double vl2 = (vx * my - vy * mx) / nrm;             // :240-241
    const double b = fabs(((vy / nrm) * q[0] + (-vx / nrm) * q[1]) + vl2);   // :243
    const double cl = norm2(mx - q[2], my - q[3]);            // :244
    const double a = sqrt(cl * cl - b * b);                   // :245
    const double t = (a * (b * b)) / cl;
    return t * t;                                             // :247
}

// :486-507 up to the counting: c.assoc[n] = the line's VP or -1.  The argmax is assign_lines' (first maximum, a NaN
// counts as the maximum); a caller's association is taken as it is, entries below 0 skip the line (:494) and entries
// of M or more -- an IndexError in the reference -- skip it too.  The outlier test reads the CALLER's s: a NaN or
// negative s[m] makes the comparison false and the line counts, as in the reference; so does a NaN distance.
template <int MEASURE>
VPK_DEVFN void vpset_assign(EmCtx& c, int M, cgdp v, cgdp s, cgllp assoc_in, double thresh) {
    const int N = c.N;
    for (int n = tid(); n < N; n += nthreads()) {
        int best = 0;
        if (assoc_in) {
            const long long a = assoc_in[n];
            best = (a < 0 || a >= M) ? -1 : (int)a;
        } else {
            double bv = c.w[n];
            for (int m = 1; m < M; ++m) {
                const double x = c.w[(size_t)m * c.ldn + n];
                if (!is_nan(bv) && (x > bv || is_nan(x))) { bv = x; best = m; }
            }
        }
        if (best >= 0) {
            const double dist = vpset_dist<MEASURE>(v + 3 * (size_t)best, c.lp + 4 * (size_t)n,
                                                    MEASURE == VPK_DIST_DOTPROD ? c.l + 3 * (size_t)n : c.lp);
            if (dist > thresh * sqrt(s[best])) best = -1;    // :504
            else if (c.lweight[n] == 0) best = -1;           // :506
        }
        c.assoc[n] = best;
    }
    block_sync();
}

// The prior of the E-step from caller-supplied cell weights (what pdf_params returns): the positive cells in index
// order, as prior_setup lists them (calc_pdf visits the cells in index order, probability_functions.py:20-21).
VPK_DEVFN void vpset_prior(const VPK_GLOBAL float* wts, double sigma) {
    Shared& sh = SH();
    for (int i = tid(); i < NCELL; i += nthreads()) sh.wts[i] = wts[i];
    block_sync();
    if (tid() == 0) {
        sh.sigma_prior = sigma;
        int nc = 0;
        for (int i = 0; i < NCELL; ++i) {
            const float w = sh.wts[i];
            if (!(w > 0)) continue;
            if (nc == MAXCOMP) { sh.flags |= VPK_VPSET_FLAG_PRIOR_TRUNCATED; break; }
            sh.pma[nc] = grid_centre(i % GRIDN);
            sh.pmb[nc] = grid_centre(i / GRIDN);
            sh.pw[nc] = (double)w;
            ++nc;
        }
        sh.ncomp = nc;
    }
    block_sync();
}

// What the EM's set-up leaves for estep / smooth, from the caller's arrays: lsim in the slot's padded layout
// (em_layout.hpp), its column sums in pairwise_setup's order (one wave per column, lanes over the rows in ascending
// order), den (:522), the zero tail rows and the per-line constants.
template <int MEASURE>
VPK_DEVFN void vpset_merge_setup(EmCtx& c, cgdp lsim, cgdp lweight) {
    Shared& sh = SH();
    const int N = c.N;
    for (int p = tid(); p < N * N; p += nthreads()) c.lsim[(size_t)(p / N) * c.ld + p % N] = lsim[p];
    for (int n = tid(); n < N; n += nthreads()) c.lweight[n] = lweight[n];
    if (tid() == 0) { sh.ibuf[2] = 0; sh.ibuf[5] = 0; }
    block_sync();
    for (int k = wave_id(); k < N; k += nwaves()) {
        double rsum = 0.0;
        for (int j = lane(); j < N; j += WAVE) rsum += c.lsim[(size_t)j * c.ld + k];
        rsum = wave_sum(rsum);
        if (lane() == 0) {
            c.rowsum[k] = rsum;
            c.den[k] = 1 + c.prm.wbias * c.lweight[k] * rsum;
            if (!(fabs(rsum) <= 1.7976931348623157e308)) sh.ibuf[2] = 1;   // (see weights_setup)
        }
    }
    block_sync();
    zero_tail_rows(c);
    line_geometry_setup<MEASURE>(c);
}

// MEASURE: distance_measure, a compile-time parameter, one kernel per measure (vpk_vpset.hip).  It reaches the outlier
// test of the counts and the E-step of a merge; split_best_vp has no measure and runs in the "angle" kernel.
template <int MEASURE>
VPK_DEV void vpset_run(const VpsetArgs& a) {
    Shared& sh = SH();
    const int b = (int)a.active[block_id()];
    const long long n0 = a.line_off[b], m0 = a.vp_off[b];
    const int N = (int)(a.line_off[b + 1] - n0), M = (int)(a.vp_off[b + 1] - m0);
    cgdp v = a.v + 3 * m0, s = a.s + m0;
    gdp ws = a.ws + a.ws_off[b];
    EmCtx c;
    c.N = N;
    c.lp = a.lp + 4 * n0;
    c.wt_doubles = a.wt_doubles;
    c.cl = nullptr;
    if (tid() == 0) { sh.M = M; sh.flags = 0; for (int q = 8; q < 16; ++q) sh.dbuf[q] = 0; }
    for (int k = tid(); k < 3 * M; k += nthreads()) { sh.cur[k] = v[k]; sh.nxt[k] = (k % 3 == 0) ? (double)(k / 3) : 0.0; }
    for (int k = tid(); k < M; k += nthreads()) sh.s[k] = s[k];
    block_sync();
    if (a.op == VPSET_MERGE) {
        c.l = (gdp)(a.l + 3 * n0);
        c.prm.use_weights = 1;
        c.prm.wbias = a.wbias;
        bind_scratch(c, (double*)ws, a.L, false);
        vpset_prior(a.prior_w + (size_t)NCELL * b, a.prior_sigma);
        vpset_merge_setup<MEASURE>(c, a.lsim + a.mat_off[b], a.lweight + n0);
        // nxt is not touched by a merge of cur, and compact_vps moves it with its VP: nxt[3 k] = the index VP k came with
        merge_vps<MEASURE>(c, false, a.thresh, a.max_stdd);
        const int Mn = sh.M;
        for (int k = tid(); k < M; k += nthreads()) {
            const bool in = k < Mn;
            for (int d = 0; d < 3; ++d) a.v_out[3 * (m0 + k) + d] = in ? sh.cur[3 * k + d] : 0.0;
            a.s_out[m0 + k] = in ? sh.s[k] : 0.0;
            a.keep_out[m0 + k] = in ? (int)sh.nxt[3 * k] : -1;
        }
        if (tid() == 0) { a.m_out[b] = Mn; a.flags_out[b] = sh.flags; }
        return;
    }
    c.ldn = N; c.ld = N; c.mcap = MAXM;                       // the caller's matrix: row stride N
    c.w = (gdp)(a.w + a.mat_off[b]);
    c.lweight = (gdp)(a.lweight + n0);
    if (a.op == VPSET_COUNTS) {
        c.assoc = (gip)ws;                                    // N ints
        if (MEASURE == VPK_DIST_DOTPROD) c.l = (gdp)(a.l + 3 * n0);
        cgllp ain = a.assoc_in ? a.assoc_in + n0 : (cgllp) nullptr;
        vpset_assign<MEASURE>(c, M, v, s, ain, a.thresh);
        count_lines(c);                                       // :509-510, the EM's summation order
        for (int k = tid(); k < M; k += nthreads()) { a.counts[m0 + k] = sh.cnt[k]; a.counts_w[m0 + k] = sh.cntw[k]; }
        for (int n = tid(); n < N; n += nthreads()) {
            long long o = c.assoc[n];
            if (ain && ain[n] < -1) o = ain[n];               // :494 leaves such an entry as it found it
            a.assoc_out[n0 + n] = o;
        }
        return;
    }
    if (MEASURE != VPK_DIST_ANGLE) return;                    // (split is launched under "angle" alone)
    // split: [cl N x N | pvl 3 N (staging of a very large set's directions) | assoc N ints | idx 3 N ints]
    c.l = (gdp)(a.l + 3 * n0);
    c.langle = (gdp)(a.langle + n0);
    c.cl = ws;
    c.pvl = ws + (size_t)N * N;
    c.assoc = (gip)(c.pvl + 3 * (size_t)N);
    c.idx = c.assoc + N;
    c.prm.merge_thresh = a.thresh;                            // min_diff (:614)
    for (int k = tid(); k < 3 * M; k += nthreads()) sh.nxt[k] = 0.0;
    block_sync();
    split_vp(c);
    const bool split = sh.M > M;                              // a VP was appended (:626-628)
    const long long o0 = m0 + b;
    for (int k = tid(); k < M + 1; k += nthreads()) {
        const bool in = k < (split ? M + 1 : M);
        for (int d = 0; d < 3; ++d) a.v_out[3 * (o0 + k) + d] = in ? (split ? sh.cur[3 * k + d] : v[3 * k + d]) : 0.0;
        a.s_out[o0 + k] = in ? (split ? sh.s[k] : s[k]) : 0.0;
    }
    if (a.labels_out)                                         // the clustering ran: 0 / 1 for the lines of the worst VP (:578)
        for (int n = tid(); n < N; n += nthreads()) a.labels_out[n0 + n] = sh.ibuf[3] >= 0 ? c.assoc[n] : -1;
    if (tid() == 0) {
        a.m_out[b] = split ? M + 1 : M;
        a.split_out[b] = split ? sh.ibuf[3] : -1;
        a.flags_out[b] = sh.flags;
    }
}

}  // namespace vpk
#endif
