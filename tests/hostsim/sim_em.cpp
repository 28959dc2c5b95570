// sim_em.cpp -- TEST-ONLY host build of the EM device source (see hip_sim.hpp): the driver em_run on one image, and the
// bodies of the library's fine-grained entry points (csrc/em_hooks.hpp, the file csrc/vpk_em.hip's fine-grained kernels call).
#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/em_hooks.hpp"

#include <stdlib.h>
#include <vector>

using namespace vpk;

static std::vector<double> g_dbg;

static void make_ctx(EmCtx& c, std::vector<double>& buf, int n, const vpk_em_params& p, bool has_init,
                     int n_init) {
    int mcap = em_mcap(p.num_init_vp, n_init, has_init, p.do_split != 0, p.num_iter, p.split_merge_freq, MAXM);
    EmLayout L = em_layout(n, mcap, 1, p.use_weights != 0, p.do_split != 0);
    buf.assign(L.total_doubles, 0.0);
    c = EmCtx{};
    c.N = n;
    c.prm = p;
    c.wt_doubles = WT_DOUBLES;
    if (const char* e = getenv("VPK_SIM_WT_DOUBLES")) c.wt_doubles = atoi(e);   // the LDS budget the phases plan with (vpk_em_set_lds_panel)
    bind_scratch(c, buf.data(), L, p.do_split != 0);
}

// the context of a fine-grained entry point: a slot for n lines and m VPs (what the hook bodies fill: em_hooks.hpp)
static void sim_hook_ctx(EmCtx& c, std::vector<double>& buf, int n, int m) {
    vpk_em_params p;
    memset(&p, 0, sizeof(p));
    p.use_weights = 1; p.num_init_vp = m; p.num_iter = 1; p.split_merge_freq = 10;
    make_ctx(c, buf, n, p, false, 0);
}

extern "C" {

int sim_em_single(int n, double* l, const double* lp, const float* cnn, const unsigned char* sphere,
                  int ssize, const double* init_vp, int n_init, const vpk_em_params* p, int max_vp,
                  double* vp_out, double* sigma_out, double* counts_out, double* counts_w_out,
                  int* num_vp_out, long long* assoc_out, int* iterations_out, int* status_out,
                  unsigned* flags_out, double* metric_out, double* trace_out) {
    EmCtx c;
    std::vector<double> buf;
    make_ctx(c, buf, n, *p, init_vp != nullptr, n_init);
    c.l = l; c.lp = lp; c.cnn = cnn; c.sphere = sphere; c.ssize = ssize;
    c.init_vp = init_vp; c.n_init = n_init;
    EmOut o;
    o.vp = vp_out; o.sigma = sigma_out; o.counts = counts_out; o.counts_w = counts_w_out;
    o.num_vp = num_vp_out; o.assoc = assoc_out; o.iterations = iterations_out; o.status = status_out;
    o.flags = flags_out; o.metric = metric_out; o.trace = trace_out; o.max_vp = max_vp;
    g_dbg.assign((size_t)p->num_iter * (1 + 4 * MAXM), 0.0);
    o.dbg = g_dbg.data();
    EmSlice sl;
    sl.deadline = EM_NO_DEADLINE;
    sl.start_iter = -1;
    if (getenv("VPK_SIM_SLICED")) {
        // time-sliced run: the stand-in clock always reads 0, so a deadline of 0 suspends the image at every
        // checkpoint; the LDS image is destroyed and the caller's l / lp arrays are poisoned between slices
        // (a suspended image must live in its slot only)
        sl.deadline = 0;
        int slices = 0;
        std::vector<double> lp_copy(lp, lp + 4 * (size_t)n);
        c.lp = lp_copy.data();
        std::vector<double> l_keep;
        while (em_run(c, o, sl) == EM_SUSPENDED) {
            memset(g_sim_lds, 0xff, sizeof(g_sim_lds));
            if (slices == 0) {
                l_keep.assign(l, l + 3 * (size_t)n);
                for (size_t q = 0; q < lp_copy.size(); ++q) lp_copy[q] = 1e300;
                for (size_t q = 0; q < 3 * (size_t)n; ++q) l[q] = -1e300;
            }
            ++slices;
        }
        if (slices) memcpy(l, l_keep.data(), l_keep.size() * sizeof(double));
        return slices;
    }
    em_run(c, o, sl);
    return 0;
}

const double* sim_last_states() { return g_dbg.data(); }

int sim_pairwise(int n, const double* lp, double* lsim_out, double* lscore_out, double* langle_out) {
    EmCtx c;
    std::vector<double> buf;
    sim_hook_ctx(c, buf, n, 25);
    hook_pairwise(c, n, lp, lsim_out, lscore_out, langle_out);
    return 0;
}

int sim_init_vps(const float* cnn, const unsigned char* sphere, int ssize, int num_max, double* v0_out,
                 int* m0_out, float* weights_out) {
    EmCtx c;
    std::vector<double> buf;
    sim_hook_ctx(c, buf, 8, num_max);
    hook_init_vps(c, cnn, sphere, ssize, num_max, v0_out, m0_out, weights_out);
    return 0;
}

int sim_estep(int n, int m, const double* lp, const float* cnn, const double* v, double* s,
              double* p_v_out, double* lvsq_out, double* p_vl_out) {
    EmCtx c;
    std::vector<double> buf;
    sim_hook_ctx(c, buf, n, m);
    hook_estep(c, n, m, lp, cnn, v, s, p_v_out, lvsq_out, p_vl_out, nullptr);
    return 0;
}

int sim_weight_matrix(int n, int m, const double* p_vl, const double* lweight, const double* lsim,
                      double bias, double* w_out) {
    EmCtx c;
    std::vector<double> buf;
    sim_hook_ctx(c, buf, n, m);
    hook_weight_matrix(c, n, m, p_vl, lweight, lsim, bias, w_out);
    return 0;
}

int sim_estep_smooth(int n, int m, const double* lp, const float* cnn, const double* v, double* s, const double* lweight,
                     const double* lsim, double bias, double* p_vl_out, double* w_out, int* info_out) {
    EmCtx c;
    std::vector<double> buf;
    sim_hook_ctx(c, buf, n, m);
    hook_estep_smooth(c, n, m, lp, cnn, v, s, lweight, lsim, bias, p_vl_out, w_out, info_out);
    return 0;
}

int sim_mstep(int n, int m, const double* l, const double* w, double* vp_out) {
    EmCtx c;
    std::vector<double> buf;
    sim_hook_ctx(c, buf, n, m);
    hook_mstep(c, n, m, l, w, vp_out, nullptr);
    return 0;
}

int sim_mstep_full(int n, int m, const double* l, const double* w, const double* lvsq, const double* p_vl, const int* assoc,
                   const double* cur, double max_stdd, double s_thresh, double* vp_out, double* s_out, double* err_out,
                   int* removed_out) {
    EmCtx c;
    std::vector<double> buf;
    sim_hook_ctx(c, buf, n, m);
    hook_mstep_full(c, n, m, l, w, lvsq, p_vl, assoc, cur, max_stdd, s_thresh, vp_out, s_out, err_out, removed_out);
    return 0;
}

int sim_line_counts(int n, int m, const double* lp, const double* v, const double* s, const double* w, const double* lweight,
                    double thresh, double* counts_out, double* counts_w_out, long long* assoc_out) {
    EmCtx c;
    std::vector<double> buf;
    sim_hook_ctx(c, buf, n, m);
    hook_line_counts(c, n, m, lp, v, s, w, lweight, thresh, counts_out, counts_w_out, assoc_out);
    return 0;
}

int sim_cluster2(int n, const double* ldist, int* labels_out, unsigned* flags_out) {
    std::vector<double> D(ldist, ldist + (size_t)n * n);   // the working copy (the library's is in its workspace)
    std::vector<int> member(n), csize(n);
    hook_cluster2(n, D.data(), member.data(), csize.data(), labels_out, flags_out);
    return 0;
}

void sim_default_params(vpk_em_params* p) {
    p->num_iter = 100; p->do_merge = 1; p->do_split = 1; p->do_iterations = 1; p->use_weights = 1;
    p->num_init_vp = 25; p->split_merge_freq = 10; p->num_min_lines = 3; p->wbias = 1.0;
    p->merge_thresh = 1e-3; p->outlier_thresh = 1.96 * 1.96; p->final_convergence = 5e-3;
    p->s_thresh = 1e-200;
}

}  // extern "C"
