// prior_device.hpp -- the CNN prior over the (alpha, beta) half sphere: pdf_params, calc_angles and calc_pdf of the
// reference's probability_functions.py as device functions.
//
// Two users: the EM workgroup (em_setup.hpp: prior_setup, and the first stage of em_estep.hpp's estep) and the stand-alone kernels of
// vpk_prior.hip (vpk_prior_params, vpk_mixture_pdf).  Written against the vocabulary of wave_prims.hpp only, so that
// tests/hostsim/sim_prior.cpp compiles it unmodified with g++ (hip_sim.hpp: one lane, WAVE = 1).  Both device units are
// compiled with -ffp-contract=off: products and sums round like the reference's separate NumPy ufunc calls.
// Citations are file:line under the reference tree.
#ifndef VPK_PRIOR_DEVICE_HPP_
#define VPK_PRIOR_DEVICE_HPP_

#include "wave_prims.hpp"

namespace vpk {

constexpr int GRIDN = 20;           // CNN output grid (cnn/deploy.prototxt:283-296)
constexpr int NCELL = GRIDN * GRIDN;
constexpr int MAXCOMP = 100;        // prior keeps the 100 strongest cells (probability_functions.py:87)
constexpr double PI_D = 3.141592653589793238462643383279502884;

VPK_DEV bool is_nan(double x) { return x != x; }
// exp for arguments that are usually far below the underflow threshold (a VP against a distant mixture
// component or line): exp(x) is exactly 0 for x < -745.14 in glibc and in ocml, so the ~50-instruction
// evaluation is skipped there -- whole waves take the short path most of the time.
VPK_DEV double exp_underflow(double x) { return x < -746.0 ? 0.0 : exp(x); }

// calc_angles (probability_functions.py:252-259) for one VP: np.minimum / np.maximum let NaN through
VPK_DEV void vp_angles(double x0, double x1, double& alpha, double& beta) {
    beta = asin(x1);
    double inner = x0 / cos(beta);
    inner = inner < 1 ? inner : (is_nan(inner) ? inner : 1.0);
    inner = inner > -1 ? inner : (is_nan(inner) ? inner : -1.0);
    alpha = asin(inner);
}

// One component of calc_pdf (:22-36) at (alpha, beta): np.sum of the five exponentials, kk = -0.5 / sigma^2 (:34).
VPK_DEV double mixture_term(double alpha, double beta, double ma, double mb, double kk) {
    double d1 = (alpha - ma) * (alpha - ma) + (beta - mb) * (beta - mb);
    double d2 = (alpha - ma + PI_D) * (alpha - ma + PI_D) + (beta + mb) * (beta + mb);
    double d3 = (alpha - ma - PI_D) * (alpha - ma - PI_D) + (beta + mb) * (beta + mb);
    double d4 = (alpha + ma) * (alpha + ma) + (beta - mb - PI_D) * (beta - mb - PI_D);
    double e4 = exp_underflow(d4 * kk);          // the fifth term duplicates the fourth (:25-26)
    return (((exp_underflow(d1 * kk) + exp_underflow(d2 * kk)) + exp_underflow(d3 * kk)) + e4) + e4;
}

// ---------------------------------------------------------------------------------------------
// pdf_params (:62-96)
// ---------------------------------------------------------------------------------------------
// numpy's float32 pairwise summation (np.sum over a contiguous float32 array), needed because
// the prior weights are normalised in float32 (probability_functions.py:82-90)
VPK_DEV float np_pairwise_block_f32(const float* a, int n) {   // 8 <= n <= 128
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i;
    for (i = 8; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}
// n = 400 splits as (96 + 104) + (96 + 104): n2 = n/2 rounded down to a multiple of 8 at each level
VPK_DEV float np_pairwise_sum_f32_400(const float* a) {
    float lo = np_pairwise_block_f32(a, 96) + np_pairwise_block_f32(a + 96, 104);
    float hi = np_pairwise_block_f32(a + 200, 96) + np_pairwise_block_f32(a + 296, 104);
    return lo + hi;
}

// np.linspace(-(A-1)/A*pi/2, (A-1)/A*pi/2, A)[i] (probability_functions.py:73,75)
VPK_DEV double grid_centre(int i) {
    double start = -(GRIDN - 1.0) / GRIDN * PI_D / 2;
    double stop = (GRIDN - 1.0) / GRIDN * PI_D / 2;
    double step = (stop - start) / (GRIDN - 1);
    return i == GRIDN - 1 ? stop : i * step + start;
}

// :82-89 for one 20 x 20 map, by the whole workgroup: wts (NCELL floats) takes the map, keep (NCELL + 1 floats) the 100
// strongest cells (the others 0) and, in keep[NCELL], their float32 sum.  wts and keep are LDS.  Ends with a barrier.
VPK_DEV void prior_keep_sum(cgfp cnn, float* wts, float* keep) {
    for (int i = tid(); i < NCELL; i += nthreads()) wts[i] = cnn[i];
    block_sync();
    for (int i = tid(); i < NCELL; i += nthreads()) {
        float wi = wts[i];
        int rank = 0;  // position in argsort(weights)[::-1]: ties -> higher index first
        for (int j = 0; j < NCELL; ++j) {
            float wj = wts[j];
            rank += (wj > wi) || (wj == wi && j > i);
        }
        keep[i] = rank < MAXCOMP ? wi : 0.f;
    }
    block_sync();
    if (tid() == 0) keep[NCELL] = np_pairwise_sum_f32_400(keep);
    block_sync();
}
// :89-90 in float32
VPK_DEV float prior_norm_f32(double sigma) { return (float)(2 * PI_D * sigma * sigma); }
VPK_DEV float prior_weight(float kept, float sum, float dv) {
    float w = kept / sum;
    return w / dv;
}

// ---------------------------------------------------------------------------------------------
// calc_pdf (:8-40) for a batch of mixtures at a set of points
// ---------------------------------------------------------------------------------------------
constexpr int PRIOR_TILE = WAVE;      // points per workgroup: one wave, one point per lane
constexpr int PRIOR_CHUNK = 128;      // components staged through LDS at a time (3 KiB)
constexpr size_t PRIOR_LDS_BYTES = 3 * PRIOR_CHUNK * sizeof(double);

struct MixtureArgs {
    int ncomp, npts;
    cgdp means;               // ncomp x 2 per image
    long long means_stride;   // doubles between images (0: one set of means for all)
    cgdp weights;             // batch x ncomp
    double kk;                // -0.5 / sigma^2
    cgdp pts;                 // npts x DIM per image
    long long pts_stride;     // doubles between images (0: one set of points for all)
    gdp angles_out;           // null or batch x npts x 2
    gdp pdf_out;              // batch x npts
};

// Tile t of image b, by a workgroup of PRIOR_TILE threads: one point per thread, every thread walks the components in index
// order and adds to ONE chain, which is calc_pdf's order (:19-38), so only exp() and the last bit of its argument separate
// the result from the reference's.  Components whose weight is not > 0 are skipped (:21; NaN weights too): the test
// is on a staged value every lane reads, so the branch is uniform.  DIM 2: the points are (alpha, beta); DIM 3: VPs,
// which go through calc_angles first.
template <int DIM> VPK_DEV void mixture_pdf_tile(const MixtureArgs& a, int b, int t) {
    double* sma = reinterpret_cast<double*>(lds_base());
    double* smb = sma + PRIOR_CHUNK;
    double* sw = smb + PRIOR_CHUNK;
    const int i = t * PRIOR_TILE + tid();
    const bool live = i < a.npts;
    double alpha = 0.0, beta = 0.0;
    if (live) {
        cgdp p = a.pts + (size_t)b * a.pts_stride + (size_t)i * DIM;
        if (DIM == 3) vp_angles(p[0], p[1], alpha, beta);
        else { alpha = p[0]; beta = p[1]; }
    }
    cgdp mean = a.means + (size_t)b * a.means_stride;
    cgdp wt = a.weights + (size_t)b * a.ncomp;
    double acc = 0.0;
    for (int c0 = 0; c0 < a.ncomp; c0 += PRIOR_CHUNK) {
        const int nc = a.ncomp - c0 < PRIOR_CHUNK ? a.ncomp - c0 : PRIOR_CHUNK;
        block_sync();                                        // the previous chunk has been read
        for (int q = tid(); q < nc; q += nthreads()) {
            sma[q] = mean[2 * (size_t)(c0 + q)];
            smb[q] = mean[2 * (size_t)(c0 + q) + 1];
            sw[q] = wt[c0 + q];
        }
        block_sync();
        if (live)
            for (int q = 0; q < nc; ++q) {
                const double w = sw[q];
                if (!(w > 0)) continue;
                acc += mixture_term(alpha, beta, sma[q], smb[q], a.kk) * w;
            }
    }
    if (live) {
        a.pdf_out[(size_t)b * a.npts + i] = acc;
        if (a.angles_out) {
            a.angles_out[2 * ((size_t)b * a.npts + i)] = alpha;
            a.angles_out[2 * ((size_t)b * a.npts + i) + 1] = beta;
        }
    }
}

}  // namespace vpk
#endif
