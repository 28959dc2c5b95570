// sim_em_estep_zeros.cpp -- TEST-ONLY host build of the EM device source (see hip_sim.hpp) with the two things sim_em.cpp and
// sim_em_measure.cpp do not hand through: EmCtx::smoother (vpk_em_set_smoother: 0 = the E-step's three passes wherever the
// panel is in LDS, 1 = the dense form they are held to) and the measure of a lone E-step + smoother.  A library of its own.
#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/em_hooks.hpp"

#include <vector>

using namespace vpk;

// em_hooks.hpp's hook_estep_smooth under either measure; the E-step's own outputs are copied out as well
template <int MEASURE>
static void estep_smooth_measure(EmCtx& c, int n, int m, const double* l, const double* lp, const float* cnn, const double* v,
                                 double* s, const double* lweight, const double* lsim, double bias, double* p_v_out,
                                 double* lvsq_out, double* p_vl_out, double* w_out, int* info_out) {
    Shared& sh = SH();
    c.N = n; c.lp = lp; c.l = const_cast<double*>(l); c.cnn = cnn;
    c.prm = vpk_em_params{};
    c.prm.use_weights = 1;
    c.prm.wbias = bias;
    prior_setup(c);
    hook_put_vps(m, v, s);
    sh.M = m;
    hook_put_lsim(c, lsim, lweight, bias);
    line_geometry_setup<MEASURE>(c);
    estep<MEASURE>(c, sh.cur);
    info_out[0] = smooth_plan(c, m);
    info_out[1] = sh.ibuf[5];
    smooth(c);
    for (int k = 0; k < m; ++k) { s[k] = sh.s[k]; p_v_out[k] = sh.pv[k]; }
    hook_get_matrix(lvsq_out, c.lvsq, c.ldn, m, n);
    hook_get_matrix(p_vl_out, c.pvl, c.ldn, m, n);
    hook_get_matrix(w_out, c.w, c.ldn, m, n);
}

extern "C" {

// l n x 3 (read under "dotprod"), lp n x 4, cnn 400, v m x 3, s m (floored in place), lweight n, lsim n x n; outputs p_v m,
// lvsq / p_vl / w [m][n], info: the smoother's plan and the panel flag the E-step left.  Returns -1 for an unknown measure.
int sim_estep_zeros(int measure, int smoother, int wt_doubles, int n, int m, const double* l, const double* lp,
                    const float* cnn, const double* v, double* s, const double* lweight, const double* lsim, double bias,
                    double* p_v_out, double* lvsq_out, double* p_vl_out, double* w_out, int* info_out) {
    vpk_em_params p;
    memset(&p, 0, sizeof(p));
    p.use_weights = 1; p.num_init_vp = m; p.num_iter = 1; p.split_merge_freq = 10;
    const int mcap = em_mcap(p.num_init_vp, 0, false, false, p.num_iter, p.split_merge_freq, MAXM);
    const EmLayout L = em_layout(n, mcap, 1, true, false);
    std::vector<double> buf(L.total_doubles, 0.0);
    EmCtx c{};
    c.N = n;
    c.prm = p;
    c.wt_doubles = wt_doubles > 0 ? wt_doubles : WT_DOUBLES;
    c.smoother = smoother;
    bind_scratch(c, buf.data(), L, false);
    if (measure == VPK_DIST_ANGLE)
        estep_smooth_measure<VPK_DIST_ANGLE>(c, n, m, l, lp, cnn, v, s, lweight, lsim, bias, p_v_out, lvsq_out, p_vl_out, w_out, info_out);
    else if (measure == VPK_DIST_DOTPROD)
        estep_smooth_measure<VPK_DIST_DOTPROD>(c, n, m, l, lp, cnn, v, s, lweight, lsim, bias, p_v_out, lvsq_out, p_vl_out, w_out, info_out);
    else
        return -1;
    return 0;
}

// the whole EM on one image (sim_em_measure.cpp's call, uninterrupted) under EmCtx::smoother; d_lvsq / d_pvl: N x max_vp each,
// the last E-step's lvsq and p_vl
int sim_em_zeros(int measure, int smoother, int wt_doubles, int n, double* l, const double* lp, const float* cnn,
                 const unsigned char* sphere, int ssize, const double* init_vp, int n_init, const vpk_em_params* p, int max_vp,
                 double* vp_out, double* sigma_out, double* counts_out, double* counts_w_out, int* num_vp_out,
                 long long* assoc_out, int* iterations_out, int* status_out, unsigned* flags_out, double* d_lvsq, double* d_pvl) {
    const bool has_init = init_vp != nullptr;
    const int mcap = em_mcap(p->num_init_vp, n_init, has_init, p->do_split != 0, p->num_iter, p->split_merge_freq, MAXM);
    const EmLayout L = em_layout(n, mcap, 1, p->use_weights != 0, p->do_split != 0);
    std::vector<double> buf(L.total_doubles, 0.0);
    EmCtx c{};
    c.N = n;
    c.prm = *p;
    c.wt_doubles = wt_doubles > 0 ? wt_doubles : WT_DOUBLES;
    c.smoother = smoother;
    bind_scratch(c, buf.data(), L, p->do_split != 0);
    c.l = l; c.lp = lp; c.cnn = cnn; c.sphere = sphere; c.ssize = ssize;
    c.init_vp = init_vp; c.n_init = n_init;
    EmOut o;
    o.vp = vp_out; o.sigma = sigma_out; o.counts = counts_out; o.counts_w = counts_w_out;
    o.num_vp = num_vp_out; o.assoc = assoc_out; o.iterations = iterations_out; o.status = status_out;
    o.flags = flags_out; o.metric = nullptr; o.trace = nullptr; o.max_vp = max_vp;
    std::vector<double> pv(max_vp), ang(2 * (size_t)max_vp), pl(n), plv((size_t)n * max_vp);
    o.d_pv = pv.data(); o.d_angles = ang.data(); o.d_pl = pl.data(); o.d_plv = plv.data();
    o.d_pvl = d_pvl; o.d_lvsq = d_lvsq;
    EmSlice sl;
    sl.deadline = EM_NO_DEADLINE;
    sl.start_iter = -1;
    if (measure == VPK_DIST_ANGLE) em_run<VPK_DIST_ANGLE>(c, o, sl);
    else if (measure == VPK_DIST_DOTPROD) em_run<VPK_DIST_DOTPROD>(c, o, sl);
    else return -1;
    return 0;
}

}  // extern "C"
