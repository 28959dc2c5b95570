// sim_vpset.cpp -- TEST-ONLY host build of vpset_device.hpp (see hip_sim.hpp): vpset_run<MEASURE> on one image, the counts
// and the merge under each of the three distance measures, with the bindings vpk_vpset.hip gives the kernel (one image, the
// active list {0}, a workspace of N ints or one EM slot).  A library of its own, as sim_em_measure.cpp is.
// With -DSIM_VPSET_MAIN the file is a program: it runs both operations under every measure on a generated image and exits
// 0 -- the form a sanitizer build takes.
#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/vpset_device.hpp"

#include <algorithm>
#include <vector>

using namespace vpk;

static int run(int measure, const VpsetArgs& a) {
    if (measure == VPK_DIST_ANGLE) vpset_run<VPK_DIST_ANGLE>(a);
    else if (measure == VPK_DIST_DOTPROD) vpset_run<VPK_DIST_DOTPROD>(a);
    else if (measure == VPK_DIST_AREA) vpset_run<VPK_DIST_AREA>(a);
    else return -1;
    return 0;
}

extern "C" {

// one image of n lines and m VPs (both > 0, m <= 64); l may be null unless measure is VPK_DIST_DOTPROD; -1: bad measure
int sim_vpset_counts(int measure, int n, int m, const double* lp, const double* l, const double* v, const double* s,
                     const double* metric, const double* lweights, double thresh, const long long* assoc_in, double* counts_out,
                     double* counts_w_out, long long* assoc_out) {
    const long long hdr[5][2] = {{0, n}, {0, m}, {0, (long long)n * m}, {0, 0}, {0, 0}};
    std::vector<double> ws((size_t)(n + 1) / 2 + 32, 0.0);
    VpsetArgs a = {};
    a.op = VPSET_COUNTS;
    a.line_off = hdr[0]; a.vp_off = hdr[1]; a.mat_off = hdr[2]; a.ws_off = hdr[3]; a.active = hdr[4];
    a.lp = lp; a.l = l; a.v = v; a.s = s; a.w = metric; a.lweight = lweights;
    a.assoc_in = assoc_in;
    a.thresh = thresh;
    a.ws = ws.data();
    a.wt_doubles = WT_DOUBLES;
    a.counts = counts_out; a.counts_w = counts_w_out; a.assoc_out = assoc_out;
    return run(measure, a);
}

// lsim: the plain n x n matrix; prior_weights: 400 cells; outputs as vpk_vp_merge_batch lays them out for one image
int sim_vpset_merge(int measure, int n, int m, const double* lp, const double* l, const double* v, const double* s,
                    const double* lweight, const double* lsim, double wbias, const float* prior_weights, double prior_sigma,
                    double thresh, double max_stdd, double* v_out, double* s_out, int* m_out, int* keep_out, unsigned* flags_out) {
    const EmLayout L = em_layout(n, (int)em_align((size_t)std::max(m, 1), 8), 1, true, false);
    const long long hdr[5][2] = {{0, n}, {0, m}, {0, (long long)n * n}, {0, (long long)L.total_doubles}, {0, 0}};
    std::vector<double> ws(L.total_doubles, 0.0);
    VpsetArgs a = {};
    a.op = VPSET_MERGE;
    a.line_off = hdr[0]; a.vp_off = hdr[1]; a.mat_off = hdr[2]; a.ws_off = hdr[3]; a.active = hdr[4];
    a.lp = lp; a.l = l; a.v = v; a.s = s; a.lweight = lweight; a.lsim = lsim;
    a.L = L;
    a.prior_w = prior_weights; a.prior_sigma = prior_sigma; a.wbias = wbias;
    a.thresh = thresh; a.max_stdd = max_stdd;
    a.ws = ws.data();
    a.wt_doubles = WT_DOUBLES;
    a.v_out = v_out; a.s_out = s_out; a.m_out = m_out; a.keep_out = keep_out; a.flags_out = flags_out;
    return run(measure, a);
}

}  // extern "C"

#ifdef SIM_VPSET_MAIN
#include <cstdio>

// a generated image: n segments aimed at one of two image points, m VPs (two of them close together), a flat prior
int main() {
    unsigned long long state = 88172645463325252ull;
    auto rnd = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0; };
    int bad = 0;
    for (int n : {1, 63, 65, 130}) {
        const int m = 3;
        const double pts[2][2] = {{0.3, -0.2}, {-0.5, 0.4}};
        std::vector<double> lp(4 * n), l(3 * n), lw(n), metric((size_t)m * n), lsim((size_t)n * n);
        for (int i = 0; i < n; ++i) {
            const double mx = 2 * rnd() - 1, my = 2 * rnd() - 1;
            const double* p = pts[i & 1];
            const double phi = atan2(p[1] - my, p[0] - mx) + 0.1 * (rnd() - 0.5), h = 0.05 + 0.15 * rnd();
            double* q = &lp[4 * i];
            q[0] = mx - h * cos(phi); q[1] = my - h * sin(phi); q[2] = mx + h * cos(phi); q[3] = my + h * sin(phi);
            double c[3] = {q[1] - q[3], q[2] - q[0], q[0] * q[3] - q[1] * q[2]};
            const double nr = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
            for (int d = 0; d < 3; ++d) l[3 * i + d] = c[d] / nr;
            lw[i] = i % 5 ? 0.2 + 0.8 * rnd() : 0.0;
            for (int k = 0; k < m; ++k) metric[(size_t)k * n + i] = rnd();
        }
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) lsim[(size_t)i * n + j] = i == j ? 0.0 : 0.5 + 0.5 * rnd();
        double v[9] = {0.3, -0.2, 1.0, -0.5, 0.4, 1.0, 0.3002, -0.2001, 1.0};
        for (int k = 0; k < m; ++k) {
            const double nr = sqrt(v[3 * k] * v[3 * k] + v[3 * k + 1] * v[3 * k + 1] + v[3 * k + 2] * v[3 * k + 2]);
            for (int d = 0; d < 3; ++d) v[3 * k + d] /= nr;
        }
        std::vector<float> prior(400, 0.0f);
        for (int q = 0; q < 400; q += 7) prior[q] = 0.01f + (float)rnd();
        for (int measure : {VPK_DIST_ANGLE, VPK_DIST_DOTPROD, VPK_DIST_AREA}) {
            const double s[3] = {1e-4, 1e-4, 1e-4};
            std::vector<double> counts(m), cw(m), v_out(3 * m), s_out(m);
            std::vector<long long> assoc(n);
            std::vector<int> keep(m);
            int m_out = -1;
            unsigned flags = 0;
            bad |= sim_vpset_counts(measure, n, m, lp.data(), l.data(), v, s, metric.data(), lw.data(), 2.57, nullptr, counts.data(),
                                    cw.data(), assoc.data());
            bad |= sim_vpset_merge(measure, n, m, lp.data(), l.data(), v, s, lw.data(), lsim.data(), 1.0, prior.data(), 0.1, 1e-3, 0.01,
                                   v_out.data(), s_out.data(), &m_out, keep.data(), &flags);
            printf("n %d measure %d: counted %g of %d, merged to %d VPs, flags %u\n", n, measure, counts[0] + counts[1] + counts[2], n,
                   m_out, flags);
            bad |= m_out < 1 || m_out > m;
        }
    }
    return bad ? 1 : 0;
}
#endif
