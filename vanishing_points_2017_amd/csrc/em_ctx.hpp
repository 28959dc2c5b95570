// em_ctx.hpp -- the EM workgroup's vocabulary: constants, the Shared block in LDS, the per-image context EmCtx and its slot binding,
// the 3-vector helpers and the workgroup-wide reductions every phase uses.
// One part of em_device.hpp (the conventions, and why the unit is compiled with -ffp-contract=off, are there).
#ifndef VPK_EM_CTX_HPP_
#define VPK_EM_CTX_HPP_

#include "wave_prims.hpp"
#include "../../include/vpk.h"
#include "em_layout.hpp"
#include "prior_device.hpp"
#include "line_device.hpp"

namespace vpk {

constexpr int MAXM = 64;            // capacity of simultaneously live VP hypotheses
constexpr int MT = 8;               // VP tile of the smoothing kernel (accumulators per column)
constexpr int PART_DOUBLES = 2048;  // LDS scratch of the setup phases (16 KiB): the head of the smoother's panel, not yet in use then
constexpr int WT_DOUBLES = 6144;    // LDS operand tile of the smoother (48 KiB)
constexpr int KNN1 = 10;            // line_rating_knn k1 (vp_localisation.py:34,230)
constexpr int TRACE_COLS = 12;       // trace row: M, max_err, M_end, events, us_estep, us_smooth, us_mstep, us_total,
                                     //            us_split_select, us_split_cluster, us_split_fit, us_merge
constexpr int KNN2 = 4;             // k2=4 at the call site (:230)

struct Shared {
    double cur[MAXM * 3];   // v[i]   of the reference's history array
    double nxt[MAXM * 3];   // v[i+1]
    double s[MAXM];         // per-VP variance
    double pv[MAXM];        // prior p(v)
    double vx[MAXM], vy[MAXM];  // VP projected to the image plane
    double k2[MAXM];        // 1 / sqrt(2 pi s)
    double cnt[MAXM], cntw[MAXM], err[MAXM];
    int removed[MAXM];
    int icnt[MAXM];
    double red_v[32];
    int red_i[32];
    double pma[MAXCOMP], pmb[MAXCOMP], pw[MAXCOMP];  // prior mixture (alpha, beta, weight)
    float wts[NCELL];
    unsigned char mx[NCELL];
    int ncomp;
    int M;
    int status;
    unsigned flags;
    int ibuf[8];
    double dbuf[16];
    double sigma_prior;
    double active_us;       // device time spent on this image in earlier time slices
};

constexpr size_t SH_BYTES = (sizeof(Shared) + 15) / 16 * 16;
static_assert(sizeof(Shared) % 8 == 0 && sizeof(Shared) <= EM_STATE_DOUBLES * 8, "Shared must fit the slot's state region");
// dynamic LDS of a launch with the default panel: [Shared | smoother operand tile]; ~77 KiB -> two workgroups per CU (160 KiB)
constexpr size_t EM_LDS_BYTES = SH_BYTES + WT_DOUBLES * sizeof(double);
// LDS layout of every EM kernel: [Shared | smoother operand panel]
VPK_DEV Shared& SH() { return *reinterpret_cast<Shared*>(lds_base()); }
VPK_DEV double* WT() { return reinterpret_cast<double*>(lds_base() + SH_BYTES); }
VPK_DEV double* SCRATCH() { return WT(); }   // PART_DOUBLES doubles; every launch gives the panel at least that much

struct EmCtx {
    int N;
    int ldn;   // row stride of the [m][n] arrays (N rounded up to 8)
    int ld;    // row stride of lsim
    int mcap;  // row stride of wsrc ([n][m]); multiple of MT
    gdp l;
    cgdp lp;
    cgfp cnn;
    cgbp sphere;
    int ssize;
    cgdp init_vp;
    int n_init;
    vpk_em_params prm;
    // per-slot global scratch
    gdp lsim;     // N x ld
    gdp pdist;    // N x ld : closest distance of every pair of segments (setup scratch)
    gdp den;      // N   : 1 + bias * lweight[k] * sum_j lsim[j][k]
    gdp lweight;  // N
    gdp langle;   // N
    gdp lscore;   // N
    gdp lvsq;     // [m][n]
    gdp pvl;      // [m][n]
    gdp w;        // [m][n]
    gdp wsrc;     // [n][mcap] : p_vl * lweight, VP index contiguous (broadcast reads)
    gdp drow;     // 6 x ldn: per-line constants of the E-step (midpoint, direction, norm) and p_l
    gdp cl;       // split: Nw x Nw cluster distances (NULL when do_split == 0)
    gip assoc;    // N
    gip idx;      // 3N (split: gathered line indices, cluster membership)
    gdp rowsum;   // N : sum_j lsim[j][k]
    int wt_doubles;   // its capacity (WT_DOUBLES, or more when the launch gives the workgroup a whole CU)
    gdp part;     // global: nwaves x mcap x ldn row-slice partial sums of the smoother
    gdp lcopy;    // N x 3 normalised lines (l points here once the setup has run)
    gdp lpcopy;   // N x 4 segment end points (lp likewise)
    gdp state;    // snapshot of Shared while the image is suspended
    int smoother = 0; // 0: the row-sliced smoother wherever it applies; 1: always the round-1/2 kernels; 2: the sparse smoother
                      // where it applies (slower, see smooth_sparse), the row-sliced one elsewhere -- same bits under all three
};

// point the context's scratch pointers into one slot
VPK_DEV void bind_scratch(EmCtx& c, double* base_, const EmLayout& L, bool do_split) {
    gdp base = (gdp)base_;
    c.ldn = L.ldn; c.ld = L.ld; c.mcap = L.mcap;
    c.lsim = base + L.lsim; c.pdist = base + L.pdist; c.den = base + L.den; c.lweight = base + L.lweight;
    c.langle = base + L.langle; c.lscore = base + L.lscore; c.lvsq = base + L.lvsq;
    c.pvl = base + L.pvl; c.w = base + L.w; c.wsrc = base + L.wsrc; c.drow = base + L.drow;
    c.cl = do_split ? base + L.cl : (gdp) nullptr;
    c.rowsum = base + L.rowsum;
    c.part = base + L.part;
    c.lcopy = base + L.lcopy; c.lpcopy = base + L.lpcopy; c.state = base + L.state;
    c.assoc = (gip)(base + L.assoc);
    c.idx = (gip)(base + L.idx);
}

// ---------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------
// (clip, dot2 and norm2: line_device.hpp)
// phase stopwatch (thread 0, after a barrier): returns microseconds since the previous call
VPK_DEV double lap(long long& t) {
    long long now = clock_ticks();
    double us = (double)(now - t) * CLOCK_US;
    t = now;
    return us;
}
// The reference's scalar code calls np.dot / np.linalg.norm on 2- and 3-vectors; NumPy's BLAS
// evaluates those as a fused chain  fma(x_{n-1}, y_{n-1}, ... fma(x1, y1, x0*y0))  (verified on the
// build container's NumPy 2.2.6 / OpenBLAS).  These helpers round the same way, which matters when a
// VP collapses onto a single line and 1 - |cos| is 0 or 1 ulp (sigma^2 at its 1e-200 floor).
VPK_DEV double dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return fma(az, bz, fma(ay, by, ax * bx));
}
VPK_DEV double norm3(double x, double y, double z) { return sqrt(dot3(x, y, z, x, y, z)); }
VPK_DEV double sign_np(double x) { return x > 0 ? 1.0 : (x < 0 ? -1.0 : (x == 0 ? 0.0 : x)); }

// workgroup-wide lexicographic (value, index) minimum; result to every thread
VPK_DEVFN void block_argmin(Shared&, double& v, int& idx) {
    Shared& sh = SH();
    wave_argmin(v, idx);
    if (lane() == 0) {
        sh.red_v[wave_id()] = v;
        sh.red_i[wave_id()] = idx;
    }
    block_sync();
    double bv = sh.red_v[0];
    int bi = sh.red_i[0];
    for (int k = 1; k < nwaves(); ++k) {
        double u = sh.red_v[k];
        int j = sh.red_i[k];
        bool take = (u < bv) || (u == bv && j < bi) || (bv != bv && u == u);
        bv = take ? u : bv;
        bi = take ? j : bi;
    }
    block_sync();
    v = bv;
    idx = bi;
}
VPK_DEVFN double block_max(Shared&, double v) {
    Shared& sh = SH();
    v = wave_max(v);
    if (lane() == 0) sh.red_v[wave_id()] = v;
    block_sync();
    double b = sh.red_v[0];
    for (int k = 1; k < nwaves(); ++k) b = nanmax(b, sh.red_v[k]);
    block_sync();
    return b;
}

}  // namespace vpk
#endif
