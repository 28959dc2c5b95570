// em_run.hpp -- the result writer, the trace, the time-slice state and the driver em_run.
// One part of em_device.hpp (the conventions, and why the unit is compiled with -ffp-contract=off, are there).
#ifndef VPK_EM_RUN_HPP_
#define VPK_EM_RUN_HPP_

#include "em_ctx.hpp"
#include "em_linalg.hpp"
#include "em_setup.hpp"
#include "em_estep.hpp"
#include "em_smooth.hpp"
#include "em_assign.hpp"
#include "em_mstep.hpp"
#include "em_vpset.hpp"

namespace vpk {

// ---------------------------------------------------------------------------------------------
// outputs
// ---------------------------------------------------------------------------------------------
struct EmOut {
    double* vp;       // max_vp x 3
    double* sigma;    // max_vp
    double* counts;   // max_vp
    double* counts_w; // max_vp
    int* num_vp;
    long long* assoc; // N
    int* iterations;
    int* status;
    unsigned* flags;
    double* metric;   // N x max_vp or null
    double* trace;    // (num_iter + 1) x TRACE_COLS or null
    int max_vp;
    double* dbg = nullptr;   // test hook: per iteration [M, s[0..MAXM), cur[0..3 MAXM)] before the E-step
    // EM_result['distribution'] (vpk_em_set_distribution_out), all null or all set
    double* d_pv = nullptr;      // max_vp
    double* d_angles = nullptr;  // max_vp x 2
    double* d_pl = nullptr;      // N
    double* d_plv = nullptr;     // N x max_vp
    double* d_pvl = nullptr;     // N x max_vp
    double* d_lvsq = nullptr;    // N x max_vp
};

VPK_DEVFN void write_result(EmCtx& c, EmOut& o, int status, int iterations) {
    Shared& sh = SH();
    const int N = c.N;
    int M = status == VPK_EM_OK ? sh.M : 0;
    if (M > o.max_vp) {
        M = o.max_vp;
        if (tid() == 0) sh.flags |= VPK_EM_FLAG_VP_OVERFLOW;
    }
    for (int m = tid(); m < o.max_vp; m += nthreads()) {
        bool ok = m < M;
        for (int d = 0; d < 3; ++d) o.vp[3 * m + d] = ok ? sh.nxt[3 * m + d] : 0.0;
        o.sigma[m] = ok ? sh.s[m] : 0.0;
        o.counts[m] = ok ? sh.cnt[m] : 0.0;
        o.counts_w[m] = ok ? sh.cntw[m] : 0.0;
    }
    for (int n = tid(); n < N; n += nthreads()) {
        int a = status == VPK_EM_OK ? c.assoc[n] : -1;
        o.assoc[n] = (a >= M) ? -1 : a;
        if (o.metric)
            for (int m = 0; m < o.max_vp; ++m)
                o.metric[(size_t)n * o.max_vp + m] = m < M ? c.w[(size_t)m * c.ldn + n] : 0.0;
    }
    if (o.d_pv) {
        // The PDF of the last calc_probabilities call (vp_localisation.py:415/:430 -> :441): lvsq and p_vl are where the last
        // E-step left them, p_lv and p_l are re-evaluated from lvsq with the E-step's expressions (it keeps their
        // product with p_v only), the angles from the VPs with the prior's (probability_functions.py:252-259).
        for (int m = tid(); m < o.max_vp; m += nthreads()) {
            const bool ok = m < M;
            double alpha = 0.0, beta = 0.0;
            if (ok) {
                const double x0 = sh.nxt[3 * m], x1 = sh.nxt[3 * m + 1];
                vp_angles(x0, x1, alpha, beta);
            }
            o.d_pv[m] = ok ? sh.pv[m] : 0.0;
            o.d_angles[2 * m] = alpha;
            o.d_angles[2 * m + 1] = beta;
        }
        for (int n = tid(); n < N; n += nthreads()) {
            double pl = 0.0;
            for (int m = 0; m < o.max_vp; ++m) {
                const bool ok = m < M;
                const double lv = ok ? c.lvsq[(size_t)m * c.ldn + n] : 0.0;
                const double plv = ok ? exp_underflow(-(lv / (2 * sh.s[m]))) * sh.k2[m] : 0.0;   // calc_plv :137-145
                if (ok) pl += plv * sh.pv[m];
                o.d_lvsq[(size_t)n * o.max_vp + m] = lv;
                o.d_plv[(size_t)n * o.max_vp + m] = plv;
                o.d_pvl[(size_t)n * o.max_vp + m] = ok ? c.pvl[(size_t)m * c.ldn + n] : 0.0;
            }
            o.d_pl[n] = (pl > 1e-12 || is_nan(pl)) ? pl : 1e-12;                                   // :116-117
        }
    }
    block_sync();
    if (tid() == 0) {
        *o.num_vp = M;
        *o.iterations = iterations;
        *o.status = status;
        *o.flags = sh.flags;
    }
    block_sync();
}

VPK_DEV void trace_put(EmOut& o, int i, int slot, double v) {
    if (o.trace && tid() == 0) o.trace[TRACE_COLS * i + slot] = v;
}
VPK_DEV void trace_add(EmOut& o, int i, int slot, double v) {
    if (o.trace && tid() == 0) o.trace[TRACE_COLS * i + slot] += v;
}


// ---------------------------------------------------------------------------------------------
// the driver: expectation_maximisation (vp_localisation.py:168-450)
// ---------------------------------------------------------------------------------------------
// Time slicing.  A launch may carry a deadline: an image that is still iterating when it passes is SUSPENDED
// at the top of its next iteration -- the only state that lives outside the slot's HBM scratch at that point
// is the Shared block in LDS, which is copied into the slot -- and resumed by a later launch (any workgroup)
// at exactly that point.  The arithmetic does not depend on where an image was suspended: results are
// bit-identical to an uninterrupted run.  Why: the EM of a never-converging image takes 99 iterations (~20 ms)
// against ~5 ms for the average one, and a launch that must run every image to completion holds its CUs for
// the slowest image.
constexpr int EM_DONE = 0, EM_SUSPENDED = 1;
constexpr long long EM_NO_DEADLINE = 0x7fffffffffffffffll;
struct EmSlice {
    long long deadline;   // clock_ticks() value; EM_NO_DEADLINE = run to completion
    int start_iter;       // in: -1 = fresh image, i >= 0 = resume at the top of iteration i; out: where it was suspended
};

VPK_DEVFN void save_state(EmCtx& c) {
    typedef VPK_GLOBAL unsigned long long* gup;
    gup dst = (gup)c.state;
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&SH());
    for (int q = tid(); q < (int)(sizeof(Shared) / 8); q += nthreads()) dst[q] = src[q];
    block_sync();
}
VPK_DEVFN void restore_state(EmCtx& c) {
    typedef const VPK_GLOBAL unsigned long long* cgup;
    cgup src = (cgup)c.state;
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(&SH());
    block_sync();
    for (int q = tid(); q < (int)(sizeof(Shared) / 8); q += nthreads()) dst[q] = src[q];
    block_sync();
}

// MEASURE: distance_measure, "angle" or "dotprod" (:196-203) -- a compile-time parameter, one kernel per measure (vpk_em.hip): it
// reaches the E-step's per-pair value, the per-line constants, the outlier test and the two start-up constants below.  The
// M-step, the smoother, split, count_lines and compaction do not see it.  A suspended image is resumed under the measure
// that suspended it (vpk_em_set_distance_measure refuses while images are parked).
template <int MEASURE = VPK_DIST_ANGLE>
VPK_DEVFN int em_run(EmCtx& c, EmOut& o, EmSlice& sl) {
    static_assert(MEASURE == VPK_DIST_ANGLE || MEASURE == VPK_DIST_DOTPROD, "the EM runs \"angle\" and \"dotprod\" (vp_localisation.py:196-203)");
    Shared& sh = SH();
    const vpk_em_params& P = c.prm;
    const double max_stdd = MEASURE == VPK_DIST_DOTPROD ? 1e-3 : 1e-6;   // :196-201 (also s_init_factor)
    const double merge_thresh_final = P.merge_thresh * 10;    // :190
    const int split_merge_it = 100;                           // :193
    long long tk = clock_ticks();
    const long long t_begin = tk;
    int first = 0;
    // w, lvsq and p_vl in the slot are those of (sh.cur, sh.s, sh.M): the iteration's E-step + smoother would write the same
    // values again and is left out.  True after the initial evaluation when the compaction behind it removed nothing
    // (never for a resumed image) and after a split event that changed nothing (split_vp); vpk_em_set_smoother(h, 1)
    // keeps every evaluation.
    bool ew_valid = false;
    if (sl.start_iter >= 0) {
        restore_state(c);
        first = sl.start_iter;
    } else {
    if (tid() == 0) { sh.flags = 0; sh.M = 0; sh.ncomp = 0; sh.ibuf[5] = 0; sh.ibuf[2] = 0; sh.active_us = 0; for (int q = 8; q < 16; ++q) sh.dbuf[q] = 0; }
    block_sync();
    if (o.trace)
        for (int q = tid(); q < TRACE_COLS * (P.num_iter + 1); q += nthreads()) o.trace[q] = 0.0;
    if (c.N <= 0) { write_result(c, o, VPK_EM_NO_VP, 0); return EM_DONE; }

    if (P.use_weights) { pairwise_setup(c, true); zero_tail_rows(c); }   // :177-178 (+ :230 kNN score)
    else pairwise_setup(c, false);                            // only lines_angles is needed
    trace_put(o, P.num_iter, 0, lap(tk));                     // last trace row: setup timings
    normalise_lines(c);                                       // :185-186, :226 (the caller's array, in place)
    for (int q = tid(); q < 3 * c.N; q += nthreads()) c.lcopy[q] = c.l[q];
    for (int q = tid(); q < 4 * c.N; q += nthreads()) c.lpcopy[q] = c.lp[q];
    block_sync();
    c.l = c.lcopy;                                            // from here on the image lives in its slot only
    c.lp = c.lpcopy;
    initial_vps(c);                                           // :208
    const int m_found = sh.M;
    prior_setup(c);                                           // :210
    if (m_found == 0) { write_result(c, o, VPK_EM_NO_INITIAL_VP, 0); return EM_DONE; }   // ValueError at :165
    if (c.init_vp) {                                          // :212-215
        if (tid() == 0) {
            int m = c.n_init < MAXM ? c.n_init : MAXM;
            for (int k = 0; k < m; ++k) {
                cgdp q = c.init_vp + 3 * (size_t)k;
                double nr = norm3(q[0], q[1], q[2]);
                sh.cur[3 * k] = q[0] / nr; sh.cur[3 * k + 1] = q[1] / nr; sh.cur[3 * k + 2] = q[2] / nr;
            }
            sh.M = m;
        }
        block_sync();
    }
    weights_setup(c);                                         // :227-235
    line_geometry_setup<MEASURE>(c);
    for (int m = tid(); m < MAXM; m += nthreads()) {
        sh.s[m] = 1.0 * (sh.sigma_prior * max_stdd);          // :219,:239 (s_init_factor == max_stdd under both measures)
        sh.nxt[3 * m] = 0; sh.nxt[3 * m + 1] = 0; sh.nxt[3 * m + 2] = 0;
    }
    block_sync();

    estep<MEASURE>(c, sh.cur);                                // :245
    smooth(c);                                                // :246
    assign_lines<MEASURE>(c, true);                           // :247
    count_lines(c);
    const int m_initial = sh.M;
    for (int m = tid(); m < sh.M; m += nthreads()) sh.removed[m] = sh.cnt[m] < 3;   // :250-251
    block_sync();
    compact_vps(c);
    ew_valid = c.smoother != 1 && sh.M == m_initial;
    trace_put(o, P.num_iter, 1, lap(tk));
    }

    for (int i = first; i < P.num_iter; ++i) {
        if (sl.deadline != EM_NO_DEADLINE && i > sl.start_iter) {   // checkpoint (at least one iteration per slice)
            if (tid() == 0) sh.ibuf[6] = clock_ticks() >= sl.deadline;
            block_sync();
            if (sh.ibuf[6]) {
                if (tid() == 0) sh.active_us += (double)(clock_ticks() - t_begin) * CLOCK_US;
                block_sync();
                save_state(c);
                sl.start_iter = i;
                return EM_SUSPENDED;
            }
        }
        tk = clock_ticks();
        const long long t_iter = tk;
        if (sh.M == 0) { write_result(c, o, VPK_EM_NO_VP, 0); return EM_DONE; }     // :258-260
        double events = 0;
        bool ew_skip = ew_valid;                              // (set for iteration 0 of a fresh image only: no split event there)
        ew_valid = false;
        if (i % P.split_merge_freq == 0 && i > 0 && i < split_merge_it && P.do_split) {   // :262-269
            int mb = sh.M;
            if (tid() == 0) { sh.dbuf[11] = 0; sh.dbuf[12] = 0; sh.dbuf[13] = 0; }
            estep<MEASURE>(c, sh.cur);
            smooth(c);
            const int wrote = split_vp(c);
            ew_skip = c.smoother != 1 && wrote == 0;
            if (sh.M != mb) events += 1;
            trace_put(o, i, 8, sh.dbuf[11]);
            trace_put(o, i, 9, sh.dbuf[12]);
            trace_put(o, i, 10, sh.dbuf[13]);
        }
        if (o.dbg && tid() == 0) {
            double* q = o.dbg + (size_t)i * (1 + 4 * MAXM);
            q[0] = sh.M;
            for (int m = 0; m < MAXM; ++m) q[1 + m] = sh.s[m];
            for (int m = 0; m < 3 * MAXM; ++m) q[1 + MAXM + m] = sh.cur[m];
        }
        lap(tk);
        if (!ew_skip) estep<MEASURE>(c, sh.cur);              // :273
        trace_put(o, i, 4, lap(tk));
        if (!ew_skip) smooth(c);                              // :282
        trace_put(o, i, 5, lap(tk));
        double max_err = 0.0;
        if (P.do_iterations) {
            mstep(c, 0, max_stdd);                            // :284-322
            trace_put(o, i, 6, lap(tk));
            max_err = max_err_of(sh, sh.M);
            block_sync();
            compact_vps(c);                                   // :329-331
        } else {
            for (int q = tid(); q < 3 * sh.M; q += nthreads()) sh.nxt[q] = sh.cur[q];   // :324-325
            block_sync();
        }
        trace_put(o, i, 0, (double)sh.M);
        trace_put(o, i, 1, max_err);
        // (:332 recomputes and discards an E-step; its only side effect, the floor of s at
        //  1e-200, cannot change s after the clamp at :307)

        if (max_err < P.final_convergence || i == P.num_iter - 1 || !P.do_iterations) {   // :335
            if (P.do_merge) merge_vps<MEASURE>(c, true, merge_thresh_final, 0.01);        // :339
            trace_put(o, P.num_iter, 3, (double)sh.M);        // finalisation audit trail: M after merge
            if (sh.M == 0) { write_result(c, o, VPK_EM_NO_VP, i); return EM_DONE; }   // reference: argmax of empty (:349)
            estep<MEASURE>(c, sh.cur);                        // :344 (stale index i)
            smooth(c);                                        // :346
            assign_lines<MEASURE>(c, false);                  // :349
            mstep(c, 1, max_stdd);                            // :353-392
            compact_vps(c);                                   // :394-396
            trace_put(o, P.num_iter, 4, (double)sh.M);        // ... after the hard-assignment M-step
            estep<MEASURE>(c, sh.cur);                        // :398 (still index i)
            smooth(c);                                        // :400
            if (sh.M == 0) { write_result(c, o, VPK_EM_NO_VP, 0); return EM_DONE; }       // :402-404
            assign_lines<MEASURE>(c, false);                  // :406
            for (int m = tid(); m < sh.M; m += nthreads()) sh.icnt[m] = 0;
            block_sync();
            for (int n = tid(); n < c.N; n += nthreads()) sh.icnt[c.assoc[n]] = 1;        // np.unique (:408)
            block_sync();
            for (int m = tid(); m < sh.M; m += nthreads()) sh.removed[m] = !sh.icnt[m];
            block_sync();
            compact_vps(c);                                   // :412-413
            trace_put(o, P.num_iter, 5, (double)sh.M);        // ... after keeping the VPs that win a line
            estep<MEASURE>(c, sh.nxt);                        // :415 (index i+1 at last)
            smooth(c);                                        // :417
            assign_lines<MEASURE>(c, true);                   // :418
            count_lines(c);
            // :423-437.  The reference's scan does NOT start over after a removal: `vidx` stays where it is (the next VP has
            // moved into that index), so a VP in front of it whose count drops below num_min_lines through the re-assignment
            // that follows a removal is never looked at again and survives with fewer lines (configs[3] image 558: a VP with
            // 2 lines in the reference's result)
            int vscan = 0;
            for (int guard = 0; guard < MAXM + 1; ++guard) {
                int vidx = -1;
                for (int m = vscan; m < sh.M; ++m)
                    if (sh.cnt[m] < P.num_min_lines) { vidx = m; break; }
                block_sync();
                if (vidx < 0) break;
                vscan = vidx;
                for (int m = tid(); m < sh.M; m += nthreads()) sh.removed[m] = (m == vidx);
                block_sync();
                compact_vps(c);
                estep<MEASURE>(c, sh.nxt);
                smooth(c);
                assign_lines<MEASURE>(c, true);
                count_lines(c);
            }
            trace_put(o, i, 2, (double)sh.M);
            trace_put(o, i, 3, events + 2);
            trace_put(o, i, 7, (double)(clock_ticks() - t_iter) * CLOCK_US);
            trace_put(o, P.num_iter, 2, sh.active_us + (double)(clock_ticks() - t_begin) * CLOCK_US);
            trace_put(o, P.num_iter, 6, sh.dbuf[8] + sh.dbuf[10]);   // smoother: operand staging + partial reduction
            trace_put(o, P.num_iter, 7, sh.dbuf[9]);                  // smoother: main loop (wave 0)
            trace_put(o, P.num_iter, 8, sh.dbuf[14]);                 // E-step: prior part
            trace_put(o, P.num_iter, 9, sh.dbuf[15]);                 // E-step: line part
            write_result(c, o, VPK_EM_OK, i);                 // :439-442
            return EM_DONE;
        }
        if (i % P.split_merge_freq == 0 && i > 0 && i <= split_merge_it + P.split_merge_freq && P.do_merge) {
            int mb = sh.M;
            lap(tk);
            merge_vps<MEASURE>(c, true, P.merge_thresh, 0.01); // :444-448
            trace_put(o, i, 11, lap(tk));
            if (sh.M != mb) events += 4;
        }
        trace_put(o, i, 2, (double)sh.M);
        trace_put(o, i, 3, events);
        trace_put(o, i, 7, (double)(clock_ticks() - t_iter) * CLOCK_US);
        for (int q = tid(); q < 3 * MAXM; q += nthreads()) {  // v[i+1] becomes v[i]; v[i+2] is zeros
            sh.cur[q] = sh.nxt[q];
            sh.nxt[q] = 0.0;
        }
        block_sync();
    }
    write_result(c, o, VPK_EM_NO_VP, 0);                      // :450
    return EM_DONE;
}

}  // namespace vpk
#endif
