// estep_device.hpp -- the E-step outside the EM: calc_probabilities (probability_functions.py:99-120) with calc_plv
// (:133-147), calc_pvl (:123-130) and the three distance measures calc_lvsq_angle (:157-176), calc_lvsq_dotprod (:150-154)
// and calc_lvsq_area (:179-209) for a ragged batch of images, any number of VPs each.
//
// One user: vpk_estep.hip (vpk_estep_batch).  The EM workgroup keeps its own E-step (em_estep.hpp: estep, em_setup.hpp:
// line_geometry_setup, "angle" and "dotprod", at most 64 VPs, fused with the smoother's panel): its per-pair expressions are
// RESTATED here operand for operand instead of shared, so that this file cannot move the EM kernel's register allocation.
// tests/test_gpu_estep_surface.py ("angle") and tests/test_gpu_em_dotprod.py ("dotprod") hold the copies together bit for bit.
//
// Written against the vocabulary of wave_prims.hpp only (through prior_device.hpp and line_device.hpp, for exp_underflow,
// is_nan, PI_D, dot2 and norm2), so that tests/hostsim/sim_estep.cpp compiles it unmodified with g++ (hip_sim.hpp: one
// lane, WAVE = 1).  Compiled with -ffp-contract=off: products and sums round like the reference's separate NumPy ufunc
// calls.  Citations are file:line under the reference tree.
#ifndef VPK_ESTEP_DEVICE_HPP_
#define VPK_ESTEP_DEVICE_HPP_

#include "wave_prims.hpp"
#include "prior_device.hpp"   // exp_underflow, is_nan, PI_D
#include "line_device.hpp"    // dot2, norm2, cglp
#include "../../include/vpk.h"   // VPK_DIST_*

namespace vpk {

constexpr int ESTEP_TILE = WAVE;      // lines per workgroup: one wave, one line per lane
constexpr int ESTEP_CHUNK = 128;      // VPs staged through LDS at a time
constexpr int ESTEP_SLOTS = 8;        // staged values per VP: five of the measure's own, 2 s, k2, p_v
constexpr size_t ESTEP_LDS_BYTES = (size_t)ESTEP_SLOTS * ESTEP_CHUNK * sizeof(double);   // 8 KiB

// Workgroups of one image.  split = false: one per tile of ESTEP_TILE lines, which walks every VP chunk in order (the p_l
// chain crosses the VPs).  split = true (no p_l, no p_vl asked for): one per (tile, chunk).  None for an empty image.
constexpr long long estep_tiles(long long n) { return (n + ESTEP_TILE - 1) / ESTEP_TILE; }
constexpr long long estep_chunks(long long m) { return (m + ESTEP_CHUNK - 1) / ESTEP_CHUNK; }
constexpr long long estep_image_blocks(long long n, long long m, bool split) {
    return (n <= 0 || m <= 0) ? 0 : estep_tiles(n) * (split ? estep_chunks(m) : 1);
}

struct EstepArgs {
    int batch;
    int split;              // the grid also splits the VP range (see estep_image_blocks)
    cglp line_off;          // batch + 1: image b's lines are [line_off[b], line_off[b + 1])
    cglp vp_off;            // batch + 1: its VPs
    cglp mat_off;           // batch + 1: its [m][n] matrices start at element mat_off[b] = sum_{a < b} M_a N_a
    cglp blk_off;           // batch + 1: its workgroups are [blk_off[b], blk_off[b + 1])
    cgdp lp;                // sum(N) x 4
    cgdp l;                 // sum(N) x 3 (dotprod only)
    cgdp v;                 // sum(M) x 3
    cgdp s;                 // sum(M)
    cgdp p_v;               // sum(M) (null when neither p_l nor p_vl is asked for)
    gdp s_out;              // sum(M): s floored at 1e-200 (:139), or null
    gdp lvsq_out;           // [m][n] per image, or null
    gdp p_lv_out;           // [m][n] per image, or null
    gdp p_l_out;            // sum(N), or null
    gdp p_vl_out;           // [m][n] per image, or null
};

// ---- the per-line constants and the per-pair distance of each measure ---------------------------------------------------
// angle: line_geometry_setup's five values (em_setup.hpp; calc_lvsq_angle :169, :172 evaluates them for every VP) --
//        midpoint, direction lp[0:2] - lp[2:4] and its norm
// area:  midpoint (:192), the first end point (:194-195) and c = |lm - lp[2:4]| (:204)
// dotprod: the homogeneous line (:151)
template <int MEASURE> VPK_DEV void estep_line(cgdp q, cgdp hl, double (&g)[5]) {
    if (MEASURE == VPK_DIST_DOTPROD) {
        g[0] = hl[0]; g[1] = hl[1]; g[2] = hl[2]; g[3] = 0.0; g[4] = 0.0;
    } else if (MEASURE == VPK_DIST_ANGLE) {
        const double v2x = q[0] - q[2], v2y = q[1] - q[3];
        g[0] = 0.5 * (q[0] + q[2]);
        g[1] = 0.5 * (q[1] + q[3]);
        g[2] = v2x;
        g[3] = v2y;
        g[4] = norm2(v2x, v2y);
    } else {
        g[0] = 0.5 * (q[0] + q[2]);
        g[1] = 0.5 * (q[1] + q[3]);
        g[2] = q[0];
        g[3] = q[1];
        g[4] = norm2(g[0] - q[2], g[1] - q[3]);
    }
}

// The VP's own values, the same expressions in every workgroup: the bits of a result do not depend on the tiling.
// angle: vx, vy (:165-166).  dotprod: v as given (:151), no division.  area: v_ = (vx, vy) (:187-188) and the part of
// vl = np.cross(v_, lmh) (:200) that no line enters: np.cross takes the 2-vector as (vx, vy, 0), so vl = (vy, -vx,
// vx my - vy mx) -- the line through the MIDPOINT in direction v_, not the line through the VP --, its norm over the first
// two components (:201) and those two divided by it.
template <int MEASURE> VPK_DEV void estep_vp(cgdp x, double (&w)[5]) {
    if (MEASURE == VPK_DIST_DOTPROD) {
        w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; w[3] = 0.0; w[4] = 0.0;
    } else {
        const double vx = x[0] / x[2], vy = x[1] / x[2];
        w[0] = vx; w[1] = vy; w[2] = 0.0; w[3] = 0.0; w[4] = 0.0;
        if (MEASURE == VPK_DIST_AREA) {
            const double nrm = norm2(vy, -vx);
            w[2] = vy / nrm;
            w[3] = -vx / nrm;
            w[4] = nrm;
        }
    }
}

template <int MEASURE> VPK_DEV double estep_lvsq(const double (&g)[5], double w0, double w1, double w2, double w3, double w4) {
    if (MEASURE == VPK_DIST_DOTPROD) {
        const double lv = (g[0] * w0 + g[1] * w1) + g[2] * w2;                 // :151
        return lv * lv;                                                        // :152
    } else if (MEASURE == VPK_DIST_ANGLE) {
        const double v1x = g[0] - w0, v1y = g[1] - w1;                         // :171
        const double n1 = norm2(v1x, v1y);
        const double cc = 1 - fabs(dot2(v1x, v1y, g[2], g[3]) / (n1 * g[4]));
        return cc * cc;                                                        // :174
    } else {
        const double vl2 = (w0 * g[1] - w1 * g[0]) / w4;                       // :200-201
        const double b = fabs((w2 * g[2] + w3 * g[3]) + vl2);                  // :203
        const double c = g[4];
        const double a = sqrt(c * c - b * b);                                  // :205 (NaN for a negative radicand, as NumPy)
        const double t = (a * (b * b)) / c;
        return t * t;                                                          // :207
    }
}

// Tile `tile` of image b over the VP chunks [c_lo, c_hi), by a workgroup of ESTEP_TILE threads: one line per thread.
// p_l (:116) is ONE chain over the VPs in ascending order of the terms p_lv p_v, floored at 1e-12 with NaN let through
// (:117, as em_estep.hpp's estep); the terms are parked in p_vl_out and divided in a second sweep (:128), in which a thread
// reads back only what it wrote itself.  Every output pointer may be null.
template <int MEASURE> VPK_DEV void estep_tile(const EstepArgs& a, int b, long long tile, int c_lo, int c_hi) {
    double* st = reinterpret_cast<double*>(lds_base());      // [ESTEP_SLOTS][ESTEP_CHUNK]
    const long long n0 = a.line_off[b], N = a.line_off[b + 1] - n0;
    const long long m0 = a.vp_off[b], M = a.vp_off[b + 1] - m0;
    const size_t mat = (size_t)a.mat_off[b];
    const long long n = tile * ESTEP_TILE + tid();
    const bool live = n < N;
    const bool chain = a.p_l_out || a.p_vl_out;
    const bool pairs = chain || a.lvsq_out || a.p_lv_out;
    if (!pairs && tile != 0) return;                         // only s_floored_out is asked for: tile 0 writes it while staging
    double g[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) estep_line<MEASURE>(a.lp + 4 * (size_t)(n0 + n), MEASURE == VPK_DIST_DOTPROD ? a.l + 3 * (size_t)(n0 + n) : a.lp, g);
    double pl = 0.0;
    for (int c = c_lo; c < c_hi; ++c) {
        const long long mc0 = (long long)c * ESTEP_CHUNK;
        const int nc = (int)(M - mc0 < ESTEP_CHUNK ? M - mc0 : ESTEP_CHUNK);
        block_sync();                                        // the previous chunk has been read
        for (int q = tid(); q < nc; q += nthreads()) {
            const size_t m = (size_t)(m0 + mc0 + q);
            double w[5];
            estep_vp<MEASURE>(a.v + 3 * m, w);
            for (int k = 0; k < 5; ++k) st[k * ESTEP_CHUNK + q] = w[k];
            double sm = a.s[m];
            sm = sm > 1e-200 ? sm : 1e-200;                  // calc_plv :139
            if (tile == 0 && a.s_out) a.s_out[m] = sm;
            st[5 * ESTEP_CHUNK + q] = 2 * sm;                // :140
            st[6 * ESTEP_CHUNK + q] = 1.0 / sqrt(2 * PI_D * sm);    // :145
            st[7 * ESTEP_CHUNK + q] = chain ? a.p_v[m] : 0.0;
        }
        block_sync();
        if (live && pairs) {
            const size_t base = mat + (size_t)mc0 * (size_t)N + (size_t)n;
#pragma unroll 4
            for (int q = 0; q < nc; ++q) {
                const double lv = estep_lvsq<MEASURE>(g, st[q], st[ESTEP_CHUNK + q], st[2 * ESTEP_CHUNK + q], st[3 * ESTEP_CHUNK + q],
                                                      st[4 * ESTEP_CHUNK + q]);
                const size_t at = base + (size_t)q * (size_t)N;
                if (a.lvsq_out) a.lvsq_out[at] = lv;
                if (a.p_lv_out || chain) {
                    const double plv = exp_underflow(-(lv / st[5 * ESTEP_CHUNK + q])) * st[6 * ESTEP_CHUNK + q];   // :137-145
                    if (a.p_lv_out) a.p_lv_out[at] = plv;
                    if (chain) {
                        const double t = plv * st[7 * ESTEP_CHUNK + q];
                        pl += t;                             // p_l = dot(p_lv, p_v) :116, in VP order
                        if (a.p_vl_out) a.p_vl_out[at] = t;
                    }
                }
            }
        }
    }
    if (chain && live) {
        pl = (pl > 1e-12 || is_nan(pl)) ? pl : 1e-12;        // :117
        if (a.p_l_out) a.p_l_out[n0 + n] = pl;
        if (a.p_vl_out) {
            const long long m_lo = (long long)c_lo * ESTEP_CHUNK;
            const long long m_hi = (long long)c_hi * ESTEP_CHUNK < M ? (long long)c_hi * ESTEP_CHUNK : M;
            for (long long m = m_lo; m < m_hi; ++m) {
                const size_t at = mat + (size_t)m * (size_t)N + (size_t)n;
                a.p_vl_out[at] = a.p_vl_out[at] / pl;        // calc_pvl :128
            }
        }
    }
}

// Workgroup `blk` of the launch: its image is the last one whose first workgroup is not past blk (images without
// workgroups share their successor's entry and are never chosen).
template <int MEASURE> VPK_DEV void estep_block(const EstepArgs& a, long long blk) {
    int lo = 0, hi = a.batch;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.blk_off[mid] <= blk) lo = mid; else hi = mid;
    }
    const long long local = blk - a.blk_off[lo];
    if (a.split) {
        const long long tiles = estep_tiles(a.line_off[lo + 1] - a.line_off[lo]);
        const int c = (int)(local / tiles);
        estep_tile<MEASURE>(a, lo, local - c * tiles, c, c + 1);
    } else {
        estep_tile<MEASURE>(a, lo, local, 0, (int)estep_chunks(a.vp_off[lo + 1] - a.vp_off[lo]));
    }
}

}  // namespace vpk
#endif
