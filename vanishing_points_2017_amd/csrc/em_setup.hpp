// em_setup.hpp -- per-image set-up phases: line normalisation, pairwise similarity and kNN score, line weights, the prior's
// parameters, the initial VPs from the CNN grid and the E-step's per-line constants.
// One part of em_device.hpp (the conventions, and why the unit is compiled with -ffp-contract=off, are there).
#ifndef VPK_EM_SETUP_HPP_
#define VPK_EM_SETUP_HPP_

#include "em_ctx.hpp"

namespace vpk {

// ---------------------------------------------------------------------------------------------
// setup: line normalisation, pairwise similarity + kNN score, weights
// ---------------------------------------------------------------------------------------------
// vp_localisation.py:185-186 and again :226 (the second pass divides by ~1)
VPK_DEVFN void normalise_lines(EmCtx& c) {
    for (int n = tid(); n < c.N; n += nthreads()) {
        gdp r = c.l + 3 * (size_t)n;
        for (int pass = 0; pass < 2; ++pass) {
            double nr = norm3(r[0], r[1], r[2]);
            r[0] /= nr; r[1] /= nr; r[2] /= nr;
        }
    }
    block_sync();
}

// calc_lsim (vp_localisation.py:87-108, sigma=1 at :178) and line_rating_knn (:34-84, k2=4 at
// :230) from ONE evaluation of every pair: the closest distance is shared by both.  Also lines_angles (:765-776).
//
// With weights (want_lsim) every UNORDERED pair is evaluated once, like the reference does (:102-108 compute
// lines_similarity(lp[i], lp[j]) for j < i and :95-97 mirror it): pass 1, one wave per row i, lanes over the
// columns j < i, writes the similarity and the distance to (i, j) and (j, i); pass 2, one wave per row, sums the
// row in the order the one-pass version did (so rowsum keeps its bits) and rates the line from its distance row.
// The pair functions are symmetric bit for bit (tests/test_gpu_em.py asserts lsim == lsim.T), so nothing moves.
// Without weights only the distances matter and the one-pass version below runs (every ordered pair, no matrix).
//
// LARGE images (N >= PW_TILED_MIN; round 6): pass 1 walks TILES of 16 rows x 64 columns instead of whole rows.  Row by row, the mirrored
// store (j, i) of a row's pairs touches N different 128-byte lines with 8 bytes each, and the other 15 entries of such a line arrive with
// the next 15 rows -- other waves, tens of microseconds later.  At N = 1000 that is 128 KB of partially written lines in flight per
// row, 256 workgroups share 32 MB of L2, the lines are evicted half-written and written again: profiles/r05_pmc_traffic.json counts
// 25.8 GB of HBM writes per 512-image stress launch against 7.6 GB algorithmic (DESIGN r5 blamed the smoother's partials,
// which N = 1000 does not have).  In a tile, one wave writes all 16 entries of a line within 16 consecutive pairs, the line is complete
// before it can be evicted, and the geometry of column j's line is computed once per 16 pairs instead of once per pair.  Same pair
// function, same argument order, same positions: every byte of lsim / pdist is the row-by-row version's (tests/test_gpu_em.py).
// The mirrored half of an interior tile goes through a wave-private LDS transpose: lane L then stores 16 bytes of row j = 8 q + L / 8 at
// columns i0 + 2 (L % 8) -- eight rows x 128 contiguous bytes per store instruction, whole lines like the direct half.  (Measured with the
// mirrored entries as 8-byte stores, 64 rows per instruction: the set-up of 256 stress images wrote 11.1 GB where the matrices are
// 4.1 GB -- profiles/r06_pmc_em_traffic.txt -- the L2 writes such sectors out more than once.)
constexpr int PW_TILED_MIN = 512;
constexpr int PW_RB = 16;                                      // rows of a tile
constexpr int PW_TLD = WAVE + 1;                               // row stride of the transpose buffers (doubles)
constexpr int PW_TBUF = 2 * PW_RB * PW_TLD;                    // per wave: similarity and distance tiles
VPK_DEV void pairwise_tiles(EmCtx& c) {
    const int N = c.N;
    double* gs = SCRATCH() + wave_id() * (PW_RB * 10);          // this wave's 16 row geometries (LineGeom = 10 doubles)
    static_assert(8 * PW_RB * 10 <= PART_DOUBLES, "row geometries of eight waves in the setup scratch");
    // the transpose buffers lie behind the setup scratch, if the launch's LDS has room for them (the whole-CU configuration has)
    const bool tbuf_ok = WAVE == 64 && PART_DOUBLES + nwaves() * PW_TBUF <= c.wt_doubles;
    double* tb = SCRATCH() + PART_DOUBLES + wave_id() * PW_TBUF;
    const int nb = (N + PW_RB - 1) / PW_RB;
    int t = 0;
    for (int I = 0; I < nb; ++I) {
        const int i0 = I * PW_RB;
        const int ilast = (i0 + PW_RB < N ? i0 + PW_RB : N) - 1;    // the block's last row; its pairs are the columns j < ilast
        const int nch = (ilast + WAVE - 1) / WAVE;
        for (int jc = 0; jc < nch; ++jc, ++t) {
            if (t % nwaves() != wave_id()) continue;            // tiles are dealt to the waves in turn
            if (lane() < PW_RB) {
                const int i = i0 + lane() < N ? i0 + lane() : N - 1;
                double a[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) a[q] = c.lp[4 * (size_t)i + q];
                const LineGeom g = line_geom(a);
                double* o = gs + lane() * 10;
                o[0] = g.x1; o[1] = g.y1; o[2] = g.x2; o[3] = g.y2; o[4] = g.dx; o[5] = g.dy; o[6] = g.nn; o[7] = g.vx; o[8] = g.vy; o[9] = g.nv;
            }
            wave_lds_order();
            const int j = jc * WAVE + lane();
            const int jj = j < N ? j : N - 1;
            double b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = c.lp[4 * (size_t)jj + q];
            const LineGeom gb = line_geom(b);
            auto row_geom = [&](int r) {
                const double* o = gs + r * 10;
                LineGeom g;
                g.x1 = o[0]; g.y1 = o[1]; g.x2 = o[2]; g.y2 = o[3]; g.dx = o[4]; g.dy = o[5]; g.nn = o[6]; g.vx = o[7]; g.vy = o[8]; g.nv = o[9];
                return g;
            };
            auto put = [&](int i, double d, double sim) {      // pair (i, j), j < i: both halves of the symmetric matrices
                if (!(j < i && i < N)) return;
                c.lsim[(size_t)i * c.ld + j] = sim;
                c.lsim[(size_t)j * c.ld + i] = sim;
                c.pdist[(size_t)i * c.ld + j] = d;
                c.pdist[(size_t)j * c.ld + i] = d;
            };
            // interior tile: every column of the chunk lies in front of the block's first row and every row exists
            const bool interior = tbuf_ok && jc * WAVE + WAVE - 1 < i0 && i0 + PW_RB <= N;
            for (int r = 0; r < PW_RB; r += 2) {                // two independent pairs per trip (see the row-by-row loop)
                const LineGeom g0 = row_geom(r), g1 = row_geom(r + 1);
                const double d0 = line_distance_closest(g0, gb);
                const double d1 = line_distance_closest(g1, gb);
                const double s0 = lines_cosangle(g0, gb, 9.0) * proximity(d0, g0.nv, gb.nv, 1.0);
                const double s1 = lines_cosangle(g1, gb, 9.0) * proximity(d1, g1.nv, gb.nv, 1.0);
                if (interior) {
                    c.lsim[(size_t)(i0 + r) * c.ld + j] = s0;   c.pdist[(size_t)(i0 + r) * c.ld + j] = d0;
                    c.lsim[(size_t)(i0 + r + 1) * c.ld + j] = s1; c.pdist[(size_t)(i0 + r + 1) * c.ld + j] = d1;
                    tb[r * PW_TLD + lane()] = s0;               tb[(PW_RB + r) * PW_TLD + lane()] = d0;
                    tb[(r + 1) * PW_TLD + lane()] = s1;         tb[(PW_RB + r + 1) * PW_TLD + lane()] = d1;
                } else {
                    put(i0 + r, d0, s0);
                    put(i0 + r + 1, d1, s1);
                }
            }
            wave_lds_order();                                   // (the next tile overwrites the row geometries)
            if (interior) {
                const int cp = lane() & 7, jr = lane() >> 3;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int jl = 8 * q + jr;                  // column of the tile = row of the mirrored entries
                    const size_t at = (size_t)(jc * WAVE + jl) * c.ld + i0 + 2 * cp;
                    store_cols2(c.lsim + at, tb[(2 * cp) * PW_TLD + jl], tb[(2 * cp + 1) * PW_TLD + jl]);
                    store_cols2(c.pdist + at, tb[(PW_RB + 2 * cp) * PW_TLD + jl], tb[(PW_RB + 2 * cp + 1) * PW_TLD + jl]);
                }
                wave_lds_order();
            }
        }
    }
    for (int i = tid(); i < N; i += nthreads()) {
        c.lsim[(size_t)i * c.ld + i] = 0.0;                     // :104 (the row's own entry stays 0)
        c.pdist[(size_t)i * c.ld + i] = 4.0;                    // :82
    }
}

VPK_DEVFN void pairwise_setup(EmCtx& c, bool want_lsim) {
    const int N = c.N;
    if (want_lsim) {
        // Row i has i pairs and row N - 1 - i has N - 1 - i: a wave takes the two together, N - 1 pairs for every
        // wave (whole trips of 2 x 64 pairs; row by row the short rows leave most lanes idle at N ~ 100..400).
        if (N >= PW_TILED_MIN && WAVE == 64 && c.smoother != 1) pairwise_tiles(c);
        else
        for (int r = wave_id(); 2 * r < N; r += nwaves()) {
            const int i0 = r, i1 = N - 1 - r;                      // i0 <= i1
            const int len = i0 == i1 ? i0 : i0 + i1;
            double a0[4], a1[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { a0[q] = c.lp[4 * (size_t)i0 + q]; a1[q] = c.lp[4 * (size_t)i1 + q]; }
            const LineGeom g0 = line_geom(a0), g1 = line_geom(a1);
            // two independent pairs per lane per trip: the per-pair arithmetic is one long dependent fp64 chain
            // (divisions, square roots, exp), so the second pair fills its issue bubbles
            auto one = [&](int t, double& d, double& sim) {
                const bool first = t < i0;
                const int j = t < len ? (first ? t : t - i0) : 0;
                const LineGeom& ga = first ? g0 : g1;              // pair (i, j): a = line i, b = line j < i (:102-106)
                double b[4] = {c.lp[4 * (size_t)j], c.lp[4 * (size_t)j + 1], c.lp[4 * (size_t)j + 2], c.lp[4 * (size_t)j + 3]};
                const LineGeom gb = line_geom(b);
                d = line_distance_closest(ga, gb);
                sim = lines_cosangle(ga, gb, 9.0) * proximity(d, ga.nv, gb.nv, 1.0);
            };
            auto put = [&](int t, double d, double sim) {
                if (t >= len) return;
                const int i = t < i0 ? i0 : i1, j = t < i0 ? t : t - i0;
                c.lsim[(size_t)i * c.ld + j] = sim;
                c.lsim[(size_t)j * c.ld + i] = sim;
                c.pdist[(size_t)i * c.ld + j] = d;
                c.pdist[(size_t)j * c.ld + i] = d;
            };
            for (int t = lane(); t < len; t += 2 * WAVE) {
                double d0, s0, d1, s1;
                one(t, d0, s0);
                one(t + WAVE, d1, s1);
                put(t, d0, s0);
                put(t + WAVE, d1, s1);
            }
            if (lane() == 0) {
                c.lsim[(size_t)i0 * c.ld + i0] = 0.0;              // :104 (the row's own entry stays 0)
                c.pdist[(size_t)i0 * c.ld + i0] = 4.0;             // :82
                c.lsim[(size_t)i1 * c.ld + i1] = 0.0;
                c.pdist[(size_t)i1 * c.ld + i1] = 4.0;
            }
        }
        block_sync();
        // pass 2a: row sums, one wave per row, each lane adds its columns in ascending order and the wave reduces --
        // the order the one-pass version used (lsim is symmetric: row sum == column sum, :522)
        for (int i = wave_id(); i < N; i += nwaves()) {
            cgdp srow = c.lsim + (size_t)i * c.ld;
            double rsum = 0.0;
            for (int j = lane(); j < N; j += WAVE) rsum += srow[j];
            rsum = wave_sum(rsum);
            if (lane() == 0) c.rowsum[i] = rsum;
        }
        // pass 2b: line_rating_knn from the stored distance rows, ROWG lanes per row and WAVE / ROWG rows per wave at a
        // time: the k1 selection rounds (a lexicographic minimum over the group and a pop) and the serial tail are
        // per-row costs that a whole wave per row paid ~14 us for; a 16-lane minimum is four DPP steps.
        constexpr int RPW = WAVE / ROWG;
        const int grp = lane() / ROWG, gl = lane() % ROWG;
        const int k1 = N < KNN1 ? N : KNN1;
        const int k2 = N < KNN2 ? N : KNN2;
        double* ks = SCRATCH() + (wave_id() * RPW + grp) * (4 * KNN1 + KNN2);   // idx, dist, cos, prox per neighbour + term by rank
        for (int base = wave_id() * RPW; base < N; base += nwaves() * RPW) {
            const int i = base + grp;
            const bool valid = i < N;
            const int ii = valid ? i : 0;
            double td[KNN1];
            int tj[KNN1];
#pragma unroll
            for (int q = 0; q < KNN1; ++q) { td[q] = 1e300; tj[q] = 0x7fffffff; }
            cgdp drow = c.pdist + (size_t)ii * c.ld;
            for (int j0 = gl; j0 < N; j0 += 4 * ROWG) {            // four loads in flight
                double dv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) dv[u] = (j0 + u * ROWG < N) ? drow[j0 + u * ROWG] : 1e300;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    double nd = dv[u];
                    int nj = (j0 + u * ROWG < N) ? j0 + u * ROWG : 0x7fffffff;
#pragma unroll
                    for (int q = 0; q < KNN1; ++q) {
                        const bool lt = (nd < td[q]) || (nd == td[q] && nj < tj[q]);
                        const double od = td[q];
                        const int oj = tj[q];
                        td[q] = lt ? nd : od;
                        tj[q] = lt ? nj : oj;
                        nd = lt ? od : nd;
                        nj = lt ? oj : nj;
                    }
                }
            }
            for (int r = 0; r < k1; ++r) {                          // k1 nearest overall, by (distance, index)
                double bd = td[0];
                int bj = tj[0];
                row16_argmin(bd, bj);
                if (tj[0] == bj && td[0] == bd) {                   // the winning lane pops its head
#pragma unroll
                    for (int q = 0; q + 1 < KNN1; ++q) { td[q] = td[q + 1]; tj[q] = tj[q + 1]; }
                    td[KNN1 - 1] = 1e300;
                    tj[KNN1 - 1] = 0x7fffffff;
                }
                if (gl == 0) { ks[r] = (double)bj; ks[KNN1 + r] = bd; }
            }
            wave_sync();
            double a[4] = {c.lp[4 * (size_t)ii], c.lp[4 * (size_t)ii + 1], c.lp[4 * (size_t)ii + 2], c.lp[4 * (size_t)ii + 3]};
            const double len_a = norm2(a[0] - a[2], a[1] - a[3]);
            for (int q = gl; q < k1; q += ROWG) {
                int j = (int)ks[q];
                j = (valid && j >= 0 && j < N) ? j : 0;
                double b[4] = {c.lp[4 * (size_t)j], c.lp[4 * (size_t)j + 1], c.lp[4 * (size_t)j + 2], c.lp[4 * (size_t)j + 3]};
                ks[2 * KNN1 + q] = lines_cosangle(a, b, 9.0);                          // :55
                // :65 lines_proximity measures the pair again: for the line itself (one of the k1 when N <= KNN1) that is
                // its distance from itself, 0 (NaN for a segment without length), not the 4 of the sorted row (:82)
                const double dq = j == ii ? line_distance_closest(a, b) : ks[KNN1 + q];
                ks[3 * KNN1 + q] = proximity(dq, len_a, line_length(b), 1.0);
            }
            wave_sync();
            // np.argsort(cosphi)[::-1][0:k2] (:57-59): descending, ties -> later position first
            for (int q = gl; q < k1; q += ROWG) {
                const double cq = ks[2 * KNN1 + q];
                int rank = 0;
                for (int p = 0; p < k1; ++p) {
                    const double cp = ks[2 * KNN1 + p];
                    rank += (cp > cq) || (cp == cq && p > q);
                }
                if (rank < k2) ks[4 * KNN1 + rank] = ks[3 * KNN1 + q] * cq;                 // :66
            }
            wave_sync();
            if (gl == 0 && valid) {
                double sum = 0.0;
                for (int r = 0; r < k2; ++r) sum += ks[4 * KNN1 + r];                       // :68, in rank order
                c.lscore[i] = sum / k2;                                                 // :70
                c.langle[i] = line_angle(a);                                            // lines_angles (:765-776)
            }
            wave_sync();
        }
        block_sync();
        return;
    }
    // per-wave kNN scratch carved from the partial-sum buffer: [k1] idx(as double), dist, cos, prox
    double* ks = SCRATCH() + wave_id() * (4 * KNN1 + KNN2);   // idx, dist, cos, prox per neighbour + term by rank
    const int k1 = N < KNN1 ? N : KNN1;
    const int k2 = N < KNN2 ? N : KNN2;
    for (int i = wave_id(); i < N; i += nwaves()) {
        double a[4] = {c.lp[4 * (size_t)i], c.lp[4 * (size_t)i + 1], c.lp[4 * (size_t)i + 2],
                       c.lp[4 * (size_t)i + 3]};
        const LineGeom ga = line_geom(a);
        const double len_a = ga.nv;               // line_length == norm of the direction (:761-762)
        double rsum = 0.0;
        // per-lane sorted list of this lane's KNN1 nearest columns, by (distance, index): filled by a
        // branch-free insertion during the pair loop, merged across the wave afterwards -- the distance
        // row never goes to memory
        double td[KNN1];
        int tj[KNN1];
#pragma unroll
        for (int q = 0; q < KNN1; ++q) { td[q] = 1e300; tj[q] = 0x7fffffff; }
        // two independent pairs per lane per trip: the per-pair arithmetic is one long dependent fp64
        // chain (divisions, square roots, exp), so the second pair fills its issue bubbles
        auto pair_eval = [&](int j, double& d, double& sim) {
            const int jj = j < N ? j : i;          // clamp: lanes past the end recompute the diagonal
            double b[4] = {c.lp[4 * (size_t)jj], c.lp[4 * (size_t)jj + 1], c.lp[4 * (size_t)jj + 2],
                           c.lp[4 * (size_t)jj + 3]};
            const LineGeom gb = line_geom(b);
            d = line_distance_closest(ga, gb);
            sim = want_lsim ? lines_cosangle(ga, gb, 9.0) * proximity(d, len_a, gb.nv, 1.0) : 0.0;
        };
        auto pair_commit = [&](int j, double d, double sim) {
            if (j >= N) return;
            if (want_lsim) {
                sim = (i == j) ? 0.0 : sim;
                c.lsim[(size_t)i * c.ld + j] = sim;
                rsum += sim;
            }
            double nd = (i == j) ? 4.0 : d;       // :82
            int nj = j;
#pragma unroll
            for (int q = 0; q < KNN1; ++q) {
                const bool lt = (nd < td[q]) || (nd == td[q] && nj < tj[q]);
                const double od = td[q];
                const int oj = tj[q];
                td[q] = lt ? nd : od;
                tj[q] = lt ? nj : oj;
                nd = lt ? od : nd;
                nj = lt ? oj : nj;
            }
        };
        for (int j = lane(); j < N; j += 2 * WAVE) {
            double d0, s0, d1, s1;
            pair_eval(j, d0, s0);
            pair_eval(j + WAVE, d1, s1);
            pair_commit(j, d0, s0);
            pair_commit(j + WAVE, d1, s1);
        }
        rsum = wave_sum(rsum);                    // lsim is symmetric: row sum == column sum (:522)
        if (lane() == 0) c.rowsum[i] = rsum;
        // k1 nearest overall: k1 rounds of lexicographic (distance, index) minimum over the lane heads
        for (int r = 0; r < k1; ++r) {
            double bd = td[0];
            int bj = tj[0];
            wave_argmin(bd, bj);
            if (tj[0] == bj && td[0] == bd) {     // the winning lane pops its head
#pragma unroll
                for (int q = 0; q + 1 < KNN1; ++q) { td[q] = td[q + 1]; tj[q] = tj[q + 1]; }
                td[KNN1 - 1] = 1e300;
                tj[KNN1 - 1] = 0x7fffffff;
            }
            if (lane() == 0) { ks[r] = (double)bj; ks[KNN1 + r] = bd; }
        }
        wave_sync();
        for (int q = lane(); q < k1; q += WAVE) {
            int j = (int)ks[q];
            double b[4] = {c.lp[4 * (size_t)j], c.lp[4 * (size_t)j + 1], c.lp[4 * (size_t)j + 2],
                           c.lp[4 * (size_t)j + 3]};
            ks[2 * KNN1 + q] = lines_cosangle(a, b, 9.0);                          // :55
            const double dq = j == i ? line_distance_closest(a, b) : ks[KNN1 + q];   // :65 (the line itself: see above)
            ks[3 * KNN1 + q] = proximity(dq, len_a, line_length(b), 1.0);
        }
        wave_sync();
        // np.argsort(cosphi)[::-1][0:k2] (:57-59): descending, ties -> later position first.  Each of the
        // k1 neighbour lanes computes its own rank; the k2 best publish prox * cos under their rank.
        for (int q = lane(); q < k1; q += WAVE) {
            const double cq = ks[2 * KNN1 + q];
            int rank = 0;
            for (int p = 0; p < k1; ++p) {
                const double cp = ks[2 * KNN1 + p];
                rank += (cp > cq) || (cp == cq && p > q);
            }
            if (rank < k2) ks[4 * KNN1 + rank] = ks[3 * KNN1 + q] * cq;                 // :66
        }
        wave_sync();
        if (lane() == 0) {
            double sum = 0.0;
            for (int r = 0; r < k2; ++r) sum += ks[4 * KNN1 + r];                       // :68, in rank order
            c.lscore[i] = sum / k2;                                                 // :70
            c.langle[i] = line_angle(a);                                            // lines_angles (:765-776)
        }
        wave_sync();
    }
    block_sync();
}

// lweight = len * clip(lscore, 0.2, 1) (vp_localisation.py:227-233) and the hoisted denominator
// of weight_matrix (:522): den[k] = 1 + bias * lweight[k] * sum_j lsim[j][k]
VPK_DEVFN void weights_setup(EmCtx& c) {
    const int N = c.N;
    const bool uw = c.prm.use_weights != 0;
    for (int n = tid(); n < N; n += nthreads()) {
        double a[4] = {c.lp[4 * (size_t)n], c.lp[4 * (size_t)n + 1], c.lp[4 * (size_t)n + 2],
                       c.lp[4 * (size_t)n + 3]};
        c.lweight[n] = uw ? line_length(a) * clip(c.lscore[n], 0.2, 1.0) : 1.0;
    }
    block_sync();
    for (int k = tid(); k < N; k += nthreads()) {
        c.den[k] = 1 + c.prm.wbias * c.lweight[k] * (uw ? c.rowsum[k] : 0.0);
        // a NaN / Inf in lsim (a segment of length 0) shows in its row sum: the sparse smoother, which leaves out the
        // terms 0 * lsim, then stands back (0 * Inf is NaN, not 0)
        if (uw && !(fabs(c.rowsum[k]) <= 1.7976931348623157e308)) SH().ibuf[2] = 1;
    }
    block_sync();
}

// ---------------------------------------------------------------------------------------------
// prior parameters and initial VPs from the CNN grid
// ---------------------------------------------------------------------------------------------
// (the float32 pairwise sum, the grid centres and the keep-100 rule itself: prior_device.hpp)
// pdf_params (probability_functions.py:62-96): keep the 100 strongest cells, normalise in f32.
VPK_DEVFN void prior_setup(EmCtx& c) {
    Shared& sh = SH();
    float* keep = (float*)SCRATCH();  // 400 floats and their sum
    if (tid() == 0) sh.sigma_prior = PI_D / (1.282 * GRIDN);  // :71
    prior_keep_sum(c.cnn, sh.wts, keep);
    // normalise every cell in parallel, then list the positive ones in cell-index order (calc_pdf visits cells in
    // index order, :20-21): position = positive cells in earlier waves + positive cells in lower lanes.  (One thread
    // walking the 400 cells with two f32 divisions each was ~50 us per image.)
    {
        const float sum = keep[NCELL];
        const float dv = prior_norm_f32(sh.sigma_prior);
        int* wcount = (int*)(SCRATCH() + 256);            // per-wave counts (behind the 401 floats)
        for (int base = 0; base < NCELL; base += nthreads()) {   // one round for 512 threads
            const int i = base + tid();
            float w = 0.f;
            if (i < NCELL) w = prior_weight(keep[i], sum, dv);
            const unsigned long long pos = wave_ballot(i < NCELL && w > 0);
            if (lane() == 0) wcount[wave_id()] = popcount64(pos);
            block_sync();
            int before = (base == 0) ? 0 : sh.ncomp;
            for (int k = 0; k < wave_id(); ++k) before += wcount[k];
            const int nc = before + popcount64(pos & lanes_below());
            if (i < NCELL) {
                sh.wts[i] = w;
                if (w > 0 && nc < MAXCOMP) {
                    sh.pma[nc] = grid_centre(i % GRIDN);   // means[:,0] = alpha, varies along columns
                    sh.pmb[nc] = grid_centre(i / GRIDN);   // means[:,1] = beta, varies along rows
                    sh.pw[nc] = (double)w;
                }
            }
            block_sync();
            if (tid() == 0) {
                int tot = before;                              // thread 0: wave 0, lane 0 -> before = carried count
                for (int k = 0; k < nwaves(); ++k) tot += wcount[k];
                sh.ncomp = tot < MAXCOMP ? tot : MAXCOMP;
            }
            block_sync();
        }
    }
}

// find_maxima (vp_localisation.py:13-31) + find_initial_vps (:111-165).  Leaves the VPs in
// sh.cur (row-major cell order), sh.M = count.  Uses SCRATCH().
VPK_DEVFN void initial_vps(EmCtx& c) {
    Shared& sh = SH();
    cgfp r = c.cnn;
    for (int i = tid(); i < NCELL; i += nthreads()) {
        int b = i / GRIDN, a = i % GRIDN;
        float vm = r[i];
        float vu = (a + 1 < GRIDN) ? r[b * GRIDN + a + 1] : 0.f;
        float vd = (a - 1 > 0) ? r[b * GRIDN + a - 1] : 0.f;   // quirk: index 0 never a neighbour
        float vl = (b - 1 > 0) ? r[(b - 1) * GRIDN + a] : 0.f;
        float vr = (b + 1 < GRIDN) ? r[(b + 1) * GRIDN + a] : 0.f;
        sh.mx[i] = (vm > vu && vm > vd && vm > vl && vm > vr) ? 1 : 0;
    }
    block_sync();
    unsigned char* keep = (unsigned char*)SCRATCH();        // 400 bytes
    double* cand = SCRATCH() + 64;                          // 400 x 4 doubles (x,y,z,valid)
    const int num_max = c.prm.num_init_vp;
    for (int i = tid(); i < NCELL; i += nthreads()) {
        int k = 0;
        if (sh.mx[i]) {
            int rank = 0;  // argsort(resp[maxima])[::-1]: ties -> later maximum first (:123-125)
            float vi = r[i];
            for (int j = 0; j < NCELL; ++j)
                if (sh.mx[j]) rank += (r[j] > vi) || (r[j] == vi && j > i);
            k = rank < num_max;
        }
        keep[i] = (unsigned char)k;
        cand[4 * i + 3] = 0.0;
    }
    block_sync();
    const int S = c.ssize;
    for (int cell = wave_id(); cell < NCELL; cell += nwaves()) {
        if (!keep[cell]) continue;
        int ra = cell / GRIDN, rb = cell % GRIDN;
        int r0 = ra * S / GRIDN, r1 = (ra + 1) * S / GRIDN;   // rows of the FLIPPED image (:114,:133)
        int c0 = rb * S / GRIDN, c1 = (rb + 1) * S / GRIDN;
        int bw = c1 - c0, npix = (r1 - r0) * bw;
        // the slice's pixels are loaded ONCE, ten per lane with all loads in flight (25 x 25 pixels at S = 500); the
        // maximum and the positions that reach it come out of registers.  (Two passes of dependent byte loads were
        // ~20 memory round trips per cell.)
        constexpr int PV = 10;
        int mxv = 0, cntp = 0, sr = 0, sc = 0;
        if (npix <= PV * WAVE) {
            int vals[PV];
#pragma unroll
            for (int q = 0; q < PV; ++q) {
                const int p = lane() + q * WAVE;
                const int pc = p < npix ? p : 0;
                const int v = c.sphere[(size_t)(S - 1 - (r0 + pc / bw)) * S + c0 + pc % bw];
                vals[q] = p < npix ? v : -1;
            }
#pragma unroll
            for (int q = 0; q < PV; ++q) mxv = vals[q] > mxv ? vals[q] : mxv;
            mxv = wave_max_int(mxv);
            if (mxv == 0) continue;                           // :137-142
#pragma unroll
            for (int q = 0; q < PV; ++q) {
                const int p = lane() + q * WAVE;
                if (vals[q] == mxv) { ++cntp; sr += p / bw; sc += p % bw; }
            }
        } else {
            for (int p = lane(); p < npix; p += WAVE) {
                int rr = r0 + p / bw, cc = c0 + p % bw;
                int v = c.sphere[(size_t)(S - 1 - rr) * S + cc];
                mxv = v > mxv ? v : mxv;
            }
            mxv = wave_max_int(mxv);
            if (mxv == 0) continue;                           // :137-142
            for (int p = lane(); p < npix; p += WAVE) {
                int rr = p / bw, cc = p % bw;
                int v = c.sphere[(size_t)(S - 1 - (r0 + rr)) * S + c0 + cc];
                if (v == mxv) { ++cntp; sr += rr; sc += cc; }
            }
        }
        cntp = wave_sum_int(cntp);
        sr = wave_sum_int(sr);
        sc = wave_sum_int(sc);
        if (lane() == 0) {
            double avg_r = (double)sr / cntp, avg_c = (double)sc / cntp;   // :148-151
            double ia = avg_c + c0, ib = avg_r + r0;                       // :155-158 (col,row)
            double alpha = (ia - 0.5 * S + 0.5) * PI_D / S;                // coordinate_conversion.py:14-15
            double beta = (ib - 0.5 * S + 0.5) * PI_D / S;
            double px = sin(alpha) * cos(beta), py = sin(beta), pz = cos(alpha) * cos(beta);
            double sg = sign_np(pz);                                       // :48
            cand[4 * cell + 0] = px * sg;
            cand[4 * cell + 1] = py * sg;
            cand[4 * cell + 2] = pz * sg;
            cand[4 * cell + 3] = 1.0;
        }
    }
    block_sync();
    if (tid() == 0) {
        int m = 0;
        for (int cell = 0; cell < NCELL; ++cell) {
            if (cand[4 * cell + 3] != 0.0 && m < MAXM) {
                sh.cur[3 * m + 0] = cand[4 * cell + 0];
                sh.cur[3 * m + 1] = cand[4 * cell + 1];
                sh.cur[3 * m + 2] = cand[4 * cell + 2];
                ++m;
            }
        }
        sh.M = m;
    }
    block_sync();
}

// Per-line constants of the E-step (calc_lvsq_angle :165-172 evaluates them again for every VP and every
// iteration): midpoint, direction and its norm, in c.drow as [5][ldn]; the line probabilities p_l of the
// current E-step follow at [5].
// "dotprod" (calc_lvsq_dotprod :151): the three components of the normalised line c.l, in the first three rows.
// "area" (calc_lvsq_area :192-204; the stand-alone merge_vps only): midpoint, first end point and c = |midpoint - second end point|.
template <int MEASURE = VPK_DIST_ANGLE>
VPK_DEVFN void line_geometry_setup(EmCtx& c) {
    for (int n = tid(); n < c.N; n += nthreads()) {
        if (MEASURE == VPK_DIST_DOTPROD) {
            cgdp q = c.l + 3 * (size_t)n;
            c.drow[n] = q[0];
            c.drow[(size_t)c.ldn + n] = q[1];
            c.drow[2 * (size_t)c.ldn + n] = q[2];
            continue;
        }
        cgdp q = c.lp + 4 * (size_t)n;
        if (MEASURE == VPK_DIST_AREA) {
            const double mx = 0.5 * (q[0] + q[2]), my = 0.5 * (q[1] + q[3]);
            c.drow[n] = mx;
            c.drow[(size_t)c.ldn + n] = my;
            c.drow[2 * (size_t)c.ldn + n] = q[0];
            c.drow[3 * (size_t)c.ldn + n] = q[1];
            c.drow[4 * (size_t)c.ldn + n] = norm2(mx - q[2], my - q[3]);
            continue;
        }
        const double v2x = q[0] - q[2], v2y = q[1] - q[3];
        c.drow[n] = 0.5 * (q[0] + q[2]);
        c.drow[(size_t)c.ldn + n] = 0.5 * (q[1] + q[3]);
        c.drow[2 * (size_t)c.ldn + n] = v2x;
        c.drow[3 * (size_t)c.ldn + n] = v2y;
        c.drow[4 * (size_t)c.ldn + n] = norm2(v2x, v2y);
    }
    block_sync();
}

}  // namespace vpk
#endif
