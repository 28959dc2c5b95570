// em_hooks.hpp -- the bodies of the fine-grained EM entry points (include/vpk.h: vpk_pairwise ... vpk_cluster2): one phase, or a
// short chain of phases, of the EM workgroup on a caller's arrays, for unit parity against the reference.
//
// Two users compile this file unmodified: vpk_em.hip (one single-workgroup kernel per function) and
// tests/hostsim/sim_em.cpp (g++ through hip_sim.hpp: one lane, WAVE = 1), so the CPU suites check the code the library runs.
// Written against the vocabulary of wave_prims.hpp only.  The phases are em_device.hpp's own -- nothing here restates one.
//
// The caller hands every function an EmCtx whose scratch is bound to a slot (bind_scratch; hook_init_vps needs none) and
// whose wt_doubles and smoother are set; the function fills the rest of the context (N, the input pointers, prm), the
// Shared block and the slot from its arguments, runs the phases and copies the outputs to the caller's arrays.  Like the
// phases, every function is called by all threads of the workgroup with uniform arguments.
#ifndef VPK_EM_HOOKS_HPP_
#define VPK_EM_HOOKS_HPP_

#include "em_device.hpp"

namespace vpk {

// ---- fillers ------------------------------------------------------------------------------------------------------
// the caller's VPs and variances into Shared (no barrier: the caller's next one publishes them)
VPK_DEV void hook_put_vps(int m, const double* v, const double* s) {
    Shared& sh = SH();
    for (int k = tid(); k < 3 * m; k += nthreads()) sh.cur[k] = v[k];
    for (int k = tid(); k < m; k += nthreads()) sh.s[k] = s[k];
}

// a caller's dense rows x cols matrix into / out of an array of row stride ld (the [m][n] arrays: ldn; lsim: ld)
VPK_DEV void hook_put_matrix(gdp dst, int ld, const double* src, int rows, int cols) {
    for (int p = tid(); p < rows * cols; p += nthreads()) dst[(size_t)(p / cols) * ld + p % cols] = src[p];
}
VPK_DEV void hook_get_matrix(double* dst, cgdp src, int ld, int rows, int cols) {
    for (int p = tid(); p < rows * cols; p += nthreads()) dst[p] = src[(size_t)(p / cols) * ld + p % cols];
}

// What the smoother needs of the set-up, from the caller's lsim (row stride n) and lweight: the matrix in padded rows with
// its zero tail, lweight, den -- a per-thread ascending sum over the caller's rows j -- and the flag for a matrix that is
// not finite (see weights_setup).  No E-step has run: the operand panel is not in LDS (sh.ibuf[5]).  Ends with a barrier.
VPK_DEV void hook_put_lsim(EmCtx& c, const double* lsim, const double* lweight, double bias) {
    Shared& sh = SH();
    const int n = c.N;
    hook_put_matrix(c.lsim, c.ld, lsim, n, n);
    for (int k = tid(); k < n; k += nthreads()) c.lweight[k] = lweight[k];
    if (tid() == 0) { sh.ibuf[5] = 0; sh.ibuf[2] = 0; }
    block_sync();
    for (int k = tid(); k < n; k += nthreads()) {
        double sum = 0.0;
        for (int j = 0; j < n; ++j) sum += lsim[(size_t)j * n + k];
        c.den[k] = 1 + bias * c.lweight[k] * sum;
        if (!(fabs(sum) <= 1.7976931348623157e308)) sh.ibuf[2] = 1;
    }
    block_sync();
    zero_tail_rows(c);
}

// ---- vpk_pairwise ---------------------------------------------------------------------------------------------------
VPK_DEV void hook_pairwise(EmCtx& c, int n, const double* lp, double* lsim_out, double* lscore_out, double* langle_out) {
    c.N = n; c.lp = (cgdp)lp;
    c.prm = vpk_em_params{};
    c.prm.use_weights = 1;
    pairwise_setup(c, true);
    hook_get_matrix(lsim_out, c.lsim, c.ld, n, n);
    for (int i = tid(); i < n; i += nthreads()) { lscore_out[i] = c.lscore[i]; langle_out[i] = c.langle[i]; }
}

// ---- vpk_init_vps (touches no scratch) ------------------------------------------------------------------------------
VPK_DEV void hook_init_vps(EmCtx& c, const float* cnn, const unsigned char* sphere, int ssize, int num_max, double* v0_out,
                           int* m0_out, float* weights_out) {
    Shared& sh = SH();
    c.N = 0; c.cnn = (cgfp)cnn; c.sphere = (cgbp)sphere; c.ssize = ssize;
    c.prm = vpk_em_params{};
    c.prm.num_init_vp = num_max;
    initial_vps(c);
    for (int k = tid(); k < 3 * sh.M; k += nthreads()) v0_out[k] = sh.cur[k];
    if (tid() == 0) *m0_out = sh.M;
    block_sync();
    prior_setup(c);
    for (int k = tid(); k < NCELL; k += nthreads()) weights_out[k] = sh.wts[k];
}

// ---- vpk_estep: lweight = 1; p_l_out may be null ----------------------------------------------------------------------
VPK_DEV void hook_estep(EmCtx& c, int n, int m, const double* lp, const float* cnn, const double* v, double* s,
                        double* p_v_out, double* lvsq_out, double* p_vl_out, double* p_l_out) {
    Shared& sh = SH();
    c.N = n; c.lp = (cgdp)lp; c.cnn = (cgfp)cnn;
    c.prm = vpk_em_params{};
    c.prm.use_weights = 1;
    prior_setup(c);
    for (int k = tid(); k < n; k += nthreads()) c.lweight[k] = 1.0;
    hook_put_vps(m, v, s);
    if (tid() == 0) sh.M = m;
    block_sync();
    line_geometry_setup(c);
    estep(c, sh.cur);
    for (int k = tid(); k < m; k += nthreads()) { s[k] = sh.s[k]; p_v_out[k] = sh.pv[k]; }
    hook_get_matrix(lvsq_out, c.lvsq, c.ldn, m, n);
    hook_get_matrix(p_vl_out, c.pvl, c.ldn, m, n);
    if (!p_l_out) return;
    // p_l is not kept by the E-step; re-evaluate sum_m p_lv * p_v with the floor (:116-117)
    for (int q = tid(); q < n; q += nthreads()) {
        double pl = 0.0;
        for (int k = 0; k < m; ++k) {
            double lv = c.lvsq[(size_t)k * c.ldn + q];
            pl += exp(-(lv / (2 * sh.s[k]))) * sh.k2[k] * sh.pv[k];
        }
        p_l_out[q] = (pl > 1e-12 || pl != pl) ? pl : 1e-12;
    }
}

// ---- vpk_weight_matrix: smooth() on a caller's p_vl; the smoother stages its panel itself ------------------------------
VPK_DEV void hook_weight_matrix(EmCtx& c, int n, int m, const double* p_vl, const double* lweight, const double* lsim,
                                double bias, double* w_out) {
    Shared& sh = SH();
    c.N = n;
    c.prm = vpk_em_params{};
    c.prm.use_weights = 1;
    c.prm.wbias = bias;
    if (tid() == 0) sh.M = m;
    hook_put_matrix(c.pvl, c.ldn, p_vl, m, n);           // (the sparse smoother's source)
    for (int p = tid(); p < n * c.mcap; p += nthreads()) {
        int i = p / c.mcap, k = p % c.mcap;
        c.wsrc[(size_t)i * c.mcap + k] = k < m ? p_vl[(size_t)k * n + i] * lweight[i] : 0.0;
    }
    hook_put_lsim(c, lsim, lweight, bias);
    smooth(c);
    hook_get_matrix(w_out, c.w, c.ldn, m, n);
}

// ---- vpk_estep_smooth: estep() followed by smooth() in ONE workgroup, so that the smoother consumes the operand panel the
// E-step left in LDS (sh.ibuf[5]) -- the batch kernel's path, which vpk_weight_matrix (panel staged by the smoother) and
// vpk_estep (lweight = 1, panel never read) do not reach.  info_out: see include/vpk.h.
VPK_DEV void hook_estep_smooth(EmCtx& c, int n, int m, const double* lp, const float* cnn, const double* v, double* s,
                               const double* lweight, const double* lsim, double bias, double* p_vl_out, double* w_out,
                               int* info_out) {
    Shared& sh = SH();
    c.N = n; c.lp = (cgdp)lp; c.cnn = (cgfp)cnn;
    c.prm = vpk_em_params{};
    c.prm.use_weights = 1;
    c.prm.wbias = bias;
    prior_setup(c);
    hook_put_vps(m, v, s);
    if (tid() == 0) sh.M = m;
    hook_put_lsim(c, lsim, lweight, bias);
    line_geometry_setup(c);
    estep(c, sh.cur);
    if (tid() == 0) {                                    // what smooth() is about to do, from its own deciding functions
        const int plan = smooth_plan(c, m);
        int wfit = ((c.wt_doubles / n) / MT) * MT;       // smooth_dispatch's pass width of smooth_full
        if (wfit > 32) wfit = 32;
        info_out[0] = plan;
        info_out[1] = sh.ibuf[5];
        info_out[2] = (sparse_smoother_fits(c) && sh.ibuf[2] == 0) ? 1 : 0;
        info_out[3] = plan == 3 ? rs_wfit(c) : wfit;
    }
    smooth(c);                                           // (nothing between the two touches the panel region)
    for (int k = tid(); k < m; k += nthreads()) s[k] = sh.s[k];
    hook_get_matrix(p_vl_out, c.pvl, c.ldn, m, n);
    hook_get_matrix(w_out, c.w, c.ldn, m, n);
}

// ---- vpk_mstep: the soft M-step from unit state; valid_out may be null -------------------------------------------------
VPK_DEV void hook_mstep(EmCtx& c, int n, int m, const double* l, const double* w, double* vp_out, int* valid_out) {
    Shared& sh = SH();
    c.N = n; c.l = (gdp) const_cast<double*>(l);
    c.prm = vpk_em_params{};
    c.prm.s_thresh = 1e-200;
    if (tid() == 0) sh.M = m;
    hook_put_matrix(c.w, c.ldn, w, m, n);
    for (int p = tid(); p < m * n; p += nthreads()) {
        int k = p / n, q = p % n;
        c.lvsq[(size_t)k * c.ldn + q] = 1.0;
        c.pvl[(size_t)k * c.ldn + q] = 1.0;
    }
    for (int k = tid(); k < 3 * m; k += nthreads()) { sh.cur[k] = (k % 3 == 2) ? 1.0 : 0.0; sh.nxt[k] = 0.0; }
    block_sync();
    mstep(c, 0, 1e-6);
    for (int k = tid(); k < m; k += nthreads()) {
        // "valid" mirrors calc_new_vanishing_point returning a vector (not None)
        bool none = sh.removed[k] && sh.err[k] == -1.0 && !(sh.s[k] != sh.s[k]);
        if (valid_out) valid_out[k] = none ? 0 : 1;
        for (int d = 0; d < 3; ++d) vp_out[3 * k + d] = none ? 0.0 : sh.nxt[3 * k + d];
    }
}

// ---- vpk_mstep_full: mstep() on caller-supplied state (assoc null: soft).  Rows the M-step does not write come back as
// vp = 0, s = -1.
VPK_DEV void hook_mstep_full(EmCtx& c, int n, int m, const double* l, const double* w, const double* lvsq,
                             const double* p_vl, const int* assoc, const double* cur, double max_stdd, double s_thresh,
                             double* vp_out, double* s_out, double* err_out, int* removed_out) {
    Shared& sh = SH();
    c.N = n; c.l = (gdp) const_cast<double*>(l);
    c.prm = vpk_em_params{};
    c.prm.s_thresh = s_thresh;
    if (tid() == 0) sh.M = m;
    hook_put_matrix(c.w, c.ldn, w, m, n);
    hook_put_matrix(c.lvsq, c.ldn, lvsq, m, n);
    hook_put_matrix(c.pvl, c.ldn, p_vl, m, n);
    if (assoc)
        for (int q = tid(); q < n; q += nthreads()) c.assoc[q] = assoc[q];
    for (int k = tid(); k < 3 * m; k += nthreads()) { sh.cur[k] = cur[k]; sh.nxt[k] = 0.0; }
    for (int k = tid(); k < m; k += nthreads()) sh.s[k] = -1.0;
    block_sync();
    mstep(c, assoc ? 1 : 0, max_stdd);
    for (int k = tid(); k < 3 * m; k += nthreads()) vp_out[k] = sh.nxt[k];
    for (int k = tid(); k < m; k += nthreads()) { s_out[k] = sh.s[k]; err_out[k] = sh.err[k]; removed_out[k] = sh.removed[k]; }
}

// ---- vpk_line_counts: calc_vp_line_counts (vp_localisation.py:482-512) on its own: argmax VP per line, the outlier test
// against calc_lvsq_single of that VP (:504) and lweight == 0 (:506), counts and weighted counts per VP.
VPK_DEV void hook_line_counts(EmCtx& c, int n, int m, const double* lp, const double* v, const double* s, const double* w,
                              const double* lweight, double thresh, double* counts_out, double* counts_w_out,
                              long long* assoc_out) {
    Shared& sh = SH();
    c.N = n; c.lp = (cgdp)lp;
    c.prm = vpk_em_params{};
    c.prm.use_weights = 1;
    c.prm.outlier_thresh = thresh;
    for (int k = tid(); k < n; k += nthreads()) c.lweight[k] = lweight[k];
    hook_put_vps(m, v, s);
    if (tid() == 0) { sh.M = m; sh.ncomp = 0; sh.sigma_prior = 1.0; }     // no prior: only lvsq is wanted from the E-step
    block_sync();
    line_geometry_setup(c);
    estep(c, sh.cur);                                                     // lvsq[m][n] (probability_functions.py:157-176)
    hook_put_matrix(c.w, c.ldn, w, m, n);
    block_sync();
    assign_lines(c, true);
    count_lines(c);
    for (int k = tid(); k < m; k += nthreads()) { counts_out[k] = sh.cnt[k]; counts_w_out[k] = sh.cntw[k]; }
    for (int k = tid(); k < n; k += nthreads()) assoc_out[k] = c.assoc[k];
}

// ---- vpk_cluster2: D is the caller's n x n working copy (destroyed), member / csize n ints each ----------------------------
// mode: EmCtx::smoother (1: the one-wave form of the LDS clustering); wt_doubles: the launch's LDS panel, as EmCtx::wt_doubles
VPK_DEV void hook_cluster2(int n, double* D, int* member, int* csize, int* labels_out, unsigned* flags_out, int mode = 0,
                           int wt_doubles = WT_DOUBLES) {
    Shared& sh = SH();
    if (tid() == 0) sh.flags = 0;
    block_sync();
    const int ld = n | 1;
    if (n <= CLUSTER_LDS_MAX && cluster_lds_doubles(n) <= wt_doubles) {   // same choice as split_vp
        double* DL = WT();
        for (int p = tid(); p < n * n; p += nthreads()) {
            const int a = p / n, b = p % n;
            const double v = D[p];
            DL[a * ld + b] = (a == b || !(v + D[(size_t)b * n + a] != 0.0)) ? -1.0 : v;
        }
        block_sync();
        cluster2_lds(n, mode);
        const int* lmember = cluster_lds_labels(DL, n);
        for (int q = tid(); q < n; q += nthreads()) member[q] = lmember[q];
        block_sync();
    } else {
        cluster2(sh, n, (gdp)D, (gip)member, (gip)csize);
    }
    for (int q = tid(); q < n; q += nthreads()) labels_out[q] = member[q];
    if (tid() == 0) *flags_out = sh.flags;
}

}  // namespace vpk
#endif
