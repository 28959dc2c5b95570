// sim_em_measure.cpp -- TEST-ONLY host build of the EM device source (see hip_sim.hpp): the driver em_run<MEASURE> on one image
// under either distance measure of the reference's EM.  A library of its own beside sim_em.cpp's (which keeps calling em_run
// without template arguments); the slicing mode is sim_em.cpp's.
#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/em_device.hpp"

#include <vector>

using namespace vpk;

template <int MEASURE>
static int run_measure(EmCtx& c, EmOut& o, int sliced, int n, double* l, const double* lp) {
    EmSlice sl;
    sl.deadline = EM_NO_DEADLINE;
    sl.start_iter = -1;
    if (!sliced) {
        em_run<MEASURE>(c, o, sl);
        return 0;
    }
    // time-sliced run: the stand-in clock always reads 0, so a deadline of 0 suspends the image at every checkpoint; the
    // LDS image is destroyed and the caller's l / lp arrays are poisoned between slices (a suspended image must live in
    // its slot only)
    sl.deadline = 0;
    int slices = 0;
    std::vector<double> lp_copy(lp, lp + 4 * (size_t)n);
    c.lp = lp_copy.data();
    std::vector<double> l_keep;
    while (em_run<MEASURE>(c, o, sl) == EM_SUSPENDED) {
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

extern "C" {

// measure: VPK_DIST_ANGLE or VPK_DIST_DOTPROD (-1 otherwise); wt_doubles: the LDS budget the phases plan with (0 = WT_DOUBLES);
// d_lvsq / d_pvl: N x max_vp each or both null (the last E-step's lvsq and p_vl, as vpk_em_set_distribution_out lays them out).
// Returns the number of slices.
int sim_em_measure(int measure, int sliced, int wt_doubles, int n, double* l, const double* lp, const float* cnn,
                   const unsigned char* sphere, int ssize, const double* init_vp, int n_init, const vpk_em_params* p,
                   int max_vp, double* vp_out, double* sigma_out, double* counts_out, double* counts_w_out, int* num_vp_out,
                   long long* assoc_out, int* iterations_out, int* status_out, unsigned* flags_out, double* d_lvsq,
                   double* d_pvl) {
    const bool has_init = init_vp != nullptr;
    const int mcap = em_mcap(p->num_init_vp, n_init, has_init, p->do_split != 0, p->num_iter, p->split_merge_freq, MAXM);
    const EmLayout L = em_layout(n, mcap, 1, p->use_weights != 0, p->do_split != 0);
    std::vector<double> buf(L.total_doubles, 0.0);
    EmCtx c{};
    c.N = n;
    c.prm = *p;
    c.wt_doubles = wt_doubles > 0 ? wt_doubles : WT_DOUBLES;
    bind_scratch(c, buf.data(), L, p->do_split != 0);
    c.l = l; c.lp = lp; c.cnn = cnn; c.sphere = sphere; c.ssize = ssize;
    c.init_vp = init_vp; c.n_init = n_init;
    EmOut o;
    o.vp = vp_out; o.sigma = sigma_out; o.counts = counts_out; o.counts_w = counts_w_out;
    o.num_vp = num_vp_out; o.assoc = assoc_out; o.iterations = iterations_out; o.status = status_out;
    o.flags = flags_out; o.metric = nullptr; o.trace = nullptr; o.max_vp = max_vp;
    std::vector<double> pv, ang, pl, plv;
    if (d_lvsq && d_pvl) {
        pv.resize(max_vp); ang.resize(2 * (size_t)max_vp); pl.resize(n); plv.resize((size_t)n * max_vp);
        o.d_pv = pv.data(); o.d_angles = ang.data(); o.d_pl = pl.data(); o.d_plv = plv.data();
        o.d_pvl = d_pvl; o.d_lvsq = d_lvsq;
    }
    if (measure == VPK_DIST_ANGLE) return run_measure<VPK_DIST_ANGLE>(c, o, sliced, n, l, lp);
    if (measure == VPK_DIST_DOTPROD) return run_measure<VPK_DIST_DOTPROD>(c, o, sliced, n, l, lp);
    return -1;
}

}  // extern "C"
