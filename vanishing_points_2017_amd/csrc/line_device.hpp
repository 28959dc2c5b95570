// line_device.hpp -- the geometry of line segments: the pair functions of the reference's vp_localisation.py:700-776
// (closest distance, the sharpened cosine, the proximity), calc_lsim (:87-108), line_rating_knn (:34-72), lines_angles
// (:765-776) and line_length (:761) as device functions.
//
// Two users: the EM workgroup (em_setup.hpp: pairwise_setup / pairwise_tiles, weights_setup) and the stand-alone batched
// kernels of vpk_lines.hip (vpk_line_similarity_batch, vpk_line_rating_batch), whose bodies are the two functions at the end
// of this file.  Written against the vocabulary of wave_prims.hpp only, so that tests/hostsim/sim_lines.cpp compiles it
// unmodified with g++ (hip_sim.hpp: one lane, WAVE = 1, ROWG = 1).  Both device units are compiled with -ffp-contract=off:
// products and sums round like the reference's separate NumPy ufunc calls.
// Citations are file:line under the reference tree.
#ifndef VPK_LINE_DEVICE_HPP_
#define VPK_LINE_DEVICE_HPP_

#include "wave_prims.hpp"
#include "prior_device.hpp"   // PI_D

namespace vpk {

VPK_DEV double clip(double x, double lo, double hi) {  // np.clip (NaN passes through)
    return x < lo ? lo : (x > hi ? hi : x);
}
// The reference's scalar code calls np.dot / np.linalg.norm on 2- and 3-vectors; NumPy's BLAS
// evaluates those as a fused chain  fma(x_{n-1}, y_{n-1}, ... fma(x1, y1, x0*y0))  (verified on the
// build container's NumPy 2.2.6 / OpenBLAS).  These helpers round the same way, which matters when a
// VP collapses onto a single line and 1 - |cos| is 0 or 1 ulp (sigma^2 at its 1e-200 floor).
VPK_DEV double dot2(double ax, double ay, double bx, double by) { return fma(ay, by, ax * bx); }
VPK_DEV double norm2(double x, double y) { return sqrt(dot2(x, y, x, y)); }

// ---------------------------------------------------------------------------------------------
// segment geometry (vp_localisation.py:700-776)
// ---------------------------------------------------------------------------------------------
// vp_localisation.py:743-758: the reference squares the NORM of (b - a) (:747)
VPK_DEV double seg_point_dist(double ax, double ay, double bx, double by, double px, double py) {
    double dx = bx - ax, dy = by - ay;
    double nrm = norm2(dx, dy);
    double param = dot2(px - ax, py - ay, dx, dy) / (nrm * nrm);
    double cx, cy;
    if (param < 0) {
        cx = ax; cy = ay;
    } else if (param > 1) {
        cx = bx; cy = by;
    } else {
        cx = ax + param * dx; cy = ay + param * dy;
    }
    double ex = cx - px, ey = cy - py;
    return norm2(ex, ey);
}
// Per-line quantities reused by every pair this line takes part in (all as the reference rounds them)
struct LineGeom {
    double x1, y1, x2, y2;   // end points
    double dx, dy;           // (x2 - x1, y2 - y1): segment vector used by line_segment_point_distance
    double nn;               // np.square(norm(d)) (:747)
    double vx, vy;           // (x1 - x2, y1 - y2): direction used by lines_points_cosangle (:716)
    double nv;               // norm(v)
};
VPK_DEV LineGeom line_geom(const double a[4]) {
    LineGeom g;
    g.x1 = a[0]; g.y1 = a[1]; g.x2 = a[2]; g.y2 = a[3];
    g.dx = a[2] - a[0]; g.dy = a[3] - a[1];
    const double nrm = norm2(g.dx, g.dy);
    g.nn = nrm * nrm;
    g.vx = a[0] - a[2]; g.vy = a[1] - a[3];
    g.nv = norm2(g.vx, g.vy);
    return g;
}
// squared distance from point p to segment s (vp_localisation.py:743-758 before the final sqrt)
VPK_DEV double seg_point_dist_sq(const LineGeom& s, double px, double py) {
    const double param = dot2(px - s.x1, py - s.y1, s.dx, s.dy) / s.nn;
    double cx, cy;
    if (param < 0) {
        cx = s.x1; cy = s.y1;
    } else if (param > 1) {
        cx = s.x2; cy = s.y2;
    } else {
        cx = s.x1 + param * s.dx; cy = s.y1 + param * s.dy;
    }
    const double ex = cx - px, ey = cy - py;
    return dot2(ex, ey, ex, ey);
}
// vp_localisation.py:727-740.  sqrt is monotonic and correctly rounded, so min(sqrt(a..d)) ==
// sqrt(min(a..d)) bit for bit: one square root per pair instead of four.
VPK_DEV double line_distance_closest(const LineGeom& a, const LineGeom& b) {
    const double d1 = seg_point_dist_sq(a, b.x1, b.y1);
    const double d2 = seg_point_dist_sq(a, b.x2, b.y2);
    const double d4 = seg_point_dist_sq(b, a.x1, a.y1);
    const double d5 = seg_point_dist_sq(b, a.x2, a.y2);
    const double m = d1 < d2 ? d1 : d2;
    const double q = d4 < d5 ? d4 : d5;
    return sqrt(m < q ? m : q);
}
// cos(clip(9 * acos(c), -pi/2, pi/2)) for c in [0, 1] without acos/cos (vp_localisation.py:721-722 with
// f = 9): with s = sin(phi) = sqrt((1 - c)(1 + c)), cos(9 phi) = Re((c + i s)^9), evaluated by repeated
// squaring (unit-modulus products: ~1e-15 absolute error, the same order as libm's last-ulp noise through
// the ill-conditioned acos near c = 1).  9 phi >= pi/2  <=>  c <= cos(pi/18): the clipped branch returns
// numpy's cos(pi/2) = 6.123233995736766e-17.
VPK_DEV double cos9_of_cos(double c) {
    const double COS_PI_18 = 0.98480775301220802;     // cos(pi / 18)
    if (!(c > COS_PI_18)) return (c != c) ? c : 6.123233995736766e-17;
    if (c > 1.0) c = 1.0;                             // np.clip(cosdphi, -1, 1)
    const double s = sqrt((1.0 - c) * (1.0 + c));
    double re = c, im = s;                            // z
    double r2 = re * re - im * im, i2 = 2 * re * im;  // z^2
    double r4 = r2 * r2 - i2 * i2, i4 = 2 * r2 * i2;  // z^4
    double r8 = r4 * r4 - i4 * i4, i8 = 2 * r4 * i4;  // z^8
    return r8 * re - i8 * im;                         // Re(z^9)
}
// (f stays a constant of the code: both callers in the reference pass 9, :55 and :701)
VPK_DEV double lines_cosangle(const LineGeom& a, const LineGeom& b, double f) {   // :715-724, f = 9 only
    const double c = fabs(dot2(a.vx, a.vy, b.vx, b.vy) / (a.nv * b.nv));
    (void)f;
    return cos9_of_cos(c);
}
// vp_localisation.py:727-740
VPK_DEV double line_distance_closest(const double a[4], const double b[4]) {
    double d1 = seg_point_dist(a[0], a[1], a[2], a[3], b[0], b[1]);
    double d2 = seg_point_dist(a[0], a[1], a[2], a[3], b[2], b[3]);
    double d4 = seg_point_dist(b[0], b[1], b[2], b[3], a[0], a[1]);
    double d5 = seg_point_dist(b[0], b[1], b[2], b[3], a[2], a[3]);
    double m = d1 < d2 ? d1 : d2;           // np.min of [d1,d2,d4,d5]; NaN handling not replicated
    double q = d4 < d5 ? d4 : d5;
    return m < q ? m : q;
}
// vp_localisation.py:715-724
VPK_DEV double lines_cosangle(const double a[4], const double b[4], double f) {
    double v1x = a[0] - a[2], v1y = a[1] - a[3];
    double v2x = b[0] - b[2], v2y = b[1] - b[3];
    double n1 = norm2(v1x, v1y), n2 = norm2(v2x, v2y);
    double c = fabs(dot2(v1x, v1y, v2x, v2y) / (n1 * n2));
    double dphi = fabs(acos(clip(c, -1.0, 1.0)));
    return cos(clip(f * dphi, -PI_D / 2, PI_D / 2));
}
VPK_DEV double line_length(const double a[4]) {
    return norm2(a[0] - a[2], a[1] - a[3]);
}
// vp_localisation.py:708-712 with the distance supplied
VPK_DEV double proximity(double d, double len_a, double len_b, double sigma) {
    double sg = sigma * (len_a < len_b ? len_a : len_b);
    return exp(-(d * d) / (2 * sg * sg));
}
// one line of lines_angles (:765-776): the angle against the x axis, folded into [0, pi/2]
VPK_DEV double line_angle(const double a[4]) {
    double vx = a[0] - a[2], vy = a[1] - a[3];
    double nr = norm2(vx, vy);
    double phi = fabs(acos(clip(vx / nr, -1.0, 1.0)));
    return phi > PI_D / 2 ? PI_D - phi : phi;
}

// ---------------------------------------------------------------------------------------------
// the batched line geometry outside the EM (vpk_lines.hip): parameters at run time, many images per launch
// ---------------------------------------------------------------------------------------------
typedef const VPK_GLOBAL long long* cglp;

struct LineBatchArgs {
    cglp offsets;        // [batch + 1]: image b's lines are lp[offsets[b] .. offsets[b + 1])
    cglp mat_offsets;    // [batch + 1]: element offset of image b's matrix in lsim (similarity only)
    cgdp lp;             // sum(N) x 4
    double sigma;
    gdp lsim;            // similarity: the matrices, row stride N_b
    int k1, k2;          // rating: 1 <= k2 <= k1 <= LR_K, clamped to N per image (:40-41)
    gdp lscore, langle, llen;   // rating: sum(N) each, any may be null
    int lds_lines;       // rating: an image of at most this many lines has its lp staged in LDS
};

// calc_lsim (:87-108) for one block of LS_RB rows of one image, by one workgroup.
//
// The walk is pairwise_tiles' (em_setup.hpp; the comment above it gives the reason): tiles of LS_RB rows x WAVE columns,
// the tile's columns over the lanes, the rows' geometries in LDS.  Every unordered pair (i, j < i) is evaluated once with
// a = line i and b = line j -- the reference's argument order (:105-106) and pairwise_setup's -- and stored to (i, j) and
// (j, i).  The direct half of a tile is 512 contiguous bytes per row and store instruction.  The mirrored half of an
// interior tile goes through a wave-private LDS transpose, so that lane L stores two adjacent entries of row
// j = 8 q + L / 8: eight rows x 128 contiguous bytes per instruction, every 128-byte line written whole by one wave within
// one tile.  The row stride is the caller's N, so the two entries are one 16-byte store only where the matrix is 16-byte
// aligned and N is even, and two 8-byte stores to the same addresses otherwise.  Edge tiles (on the diagonal, in a last
// row block that is not full, in a last column chunk past N) store entry by entry, guarded.  The blocks of an image are
// numbered from its LAST rows: those have the most pairs and start first.  Nothing but lsim is written: no distances.
constexpr int LS_RB = 16;                                      // rows of a tile
constexpr int LS_TLD = WAVE + 1;                               // row stride of the transpose buffer (doubles)
constexpr int LS_WAVE_DOUBLES = LS_RB * 10 + LS_RB * LS_TLD;   // per wave: 16 row geometries (LineGeom = 10 doubles) + one tile
VPK_DEV void line_similarity_rowblock(const LineBatchArgs& A, int img, int blk) {
    const long long o0 = A.offsets[img];
    const int N = uniform_int((int)(A.offsets[img + 1] - o0));
    const int nb = (N + LS_RB - 1) / LS_RB;
    if (blk >= nb) return;
    const int i0 = (nb - 1 - blk) * LS_RB;
    cgdp lp = A.lp + 4 * o0;
    gdp S = A.lsim + A.mat_offsets[img];
    const int wv = uniform_int(wave_id());
    double* gs = reinterpret_cast<double*>(lds_base()) + wv * LS_WAVE_DOUBLES;
    double* tb = gs + LS_RB * 10;
    const int ilast = (i0 + LS_RB < N ? i0 + LS_RB : N) - 1;   // the block's last row; its pairs are the columns j < ilast
    const int nch = (ilast + WAVE - 1) / WAVE;
    const bool store16 = (N & 1) == 0 && ((unsigned long long)S & 15ull) == 0;
    for (int r = lane(); r < LS_RB; r += WAVE) {                // the same 16 rows for every tile of this wave
        const int i = i0 + r < N ? i0 + r : N - 1;
        double a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = lp[4 * (size_t)i + q];
        const LineGeom g = line_geom(a);
        double* o = gs + r * 10;
        o[0] = g.x1; o[1] = g.y1; o[2] = g.x2; o[3] = g.y2; o[4] = g.dx; o[5] = g.dy; o[6] = g.nn; o[7] = g.vx; o[8] = g.vy; o[9] = g.nv;
    }
    wave_lds_order();
    auto row_geom = [&](int r) {
        const double* o = gs + r * 10;
        LineGeom g;
        g.x1 = o[0]; g.y1 = o[1]; g.x2 = o[2]; g.y2 = o[3]; g.dx = o[4]; g.dy = o[5]; g.nn = o[6]; g.vx = o[7]; g.vy = o[8]; g.nv = o[9];
        return g;
    };
    for (int jc = wv; jc < nch; jc += nwaves()) {               // the block's column chunks are dealt to the waves in turn
        const int j = jc * WAVE + lane();
        const int jj = j < N ? j : N - 1;
        double b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = lp[4 * (size_t)jj + q];
        const LineGeom gb = line_geom(b);
        auto put = [&](int i, double sim) {                     // pair (i, j), j < i: both halves of the symmetric matrix
            if (!(j < i && i < N)) return;
            S[(size_t)i * N + j] = sim;
            S[(size_t)j * N + i] = sim;
        };
        // interior tile: every column of the chunk lies in front of the block's first row and every row exists
        const bool interior = WAVE == 64 && jc * WAVE + WAVE - 1 < i0 && i0 + LS_RB <= N;
        for (int r = 0; r < LS_RB; r += 2) {                    // two independent pairs per trip: each is one long fp64 chain
            const LineGeom g0 = row_geom(r), g1 = row_geom(r + 1);
            const double d0 = line_distance_closest(g0, gb);
            const double d1 = line_distance_closest(g1, gb);
            const double s0 = lines_cosangle(g0, gb, 9.0) * proximity(d0, g0.nv, gb.nv, A.sigma);
            const double s1 = lines_cosangle(g1, gb, 9.0) * proximity(d1, g1.nv, gb.nv, A.sigma);
            if (interior) {
                S[(size_t)(i0 + r) * N + j] = s0;
                S[(size_t)(i0 + r + 1) * N + j] = s1;
                tb[r * LS_TLD + lane()] = s0;
                tb[(r + 1) * LS_TLD + lane()] = s1;
            } else {
                put(i0 + r, s0);
                put(i0 + r + 1, s1);
            }
        }
        if (interior) {
            wave_lds_order();
            const int cp = lane() & 7, jr = lane() >> 3;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int jl = 8 * q + jr;                      // column of the tile = row of the mirrored entries
                const size_t at = (size_t)(jc * WAVE + jl) * N + i0 + 2 * cp;
                const double e0 = tb[(2 * cp) * LS_TLD + jl], e1 = tb[(2 * cp + 1) * LS_TLD + jl];
                if (store16) store_cols2(S + at, e0, e1);
                else { S[at] = e0; S[at + 1] = e1; }
            }
            wave_lds_order();                                   // (the next tile overwrites the transpose buffer)
        }
    }
    if (wv == 0)
        for (int r = lane(); r < LS_RB; r += WAVE)
            if (i0 + r < N) S[(size_t)(i0 + r) * N + i0 + r] = 0.0;   // :104 (the row's own entry stays 0)
}

// line_rating_knn (:34-72, before any clip), lines_angles (:765-776) and line_length (:761) for nthreads() / ROWG rows of
// one image, by one workgroup, without a distance matrix.
//
// ROWG lanes per row, as pass 2b of pairwise_setup.  Each lane evaluates the closest distance from its row to its columns
// j = lane, lane + ROWG, ... on the fly and keeps the LR_K smallest (distance, index) pairs in registers (a predicated
// compare-exchange chain, fully unrolled: no indexed register access); the group then takes k1 rounds of a lexicographic
// minimum over the lanes' heads.  From there on the code is pass 2b's with k1, k2 and sigma as values: cosines and
// proximities of the k1 neighbours, the k2 largest cosines (among equal ones the later position first: argsort(...)[::-1],
// :57-59), their products summed in rank order and divided by the clamped k2 (:70).  The row itself enters with distance 4
// (:82); where it is among the k1, its proximity is measured again from its distance to itself (:65).
// The distance of the pair (i, j) is taken with a = the line of the LARGER index: that is the one evaluation the
// similarity's lower triangle makes and pairwise_setup mirrors into its distance matrix, so a NaN takes the same way
// through the minima and the bits are those of the EM's pass.
// STAGED: the image's lp (32 N bytes) lies in LDS behind the groups' scratch; otherwise every read goes to L2.
constexpr int LR_K = 16;                 // capacity of the neighbour lists: k1 <= LR_K
constexpr int LR_KS = 5 * LR_K;          // per row group: idx, dist, cos, prox per neighbour + term by rank
template <bool STAGED>
VPK_DEV void line_rating_rows(const LineBatchArgs& A, int img, int blk) {
    const long long o0 = A.offsets[img];
    const int N = uniform_int((int)(A.offsets[img + 1] - o0));
    const int rpb = nthreads() / ROWG;   // rows per workgroup
    if ((long long)blk * rpb >= N) return;
    cgdp lp = A.lp + 4 * o0;
    double* lds = reinterpret_cast<double*>(lds_base());
    const double* slp = lds + rpb * LR_KS;
    if (STAGED) {
        for (int q = tid(); q < 4 * N; q += nthreads()) lds[rpb * LR_KS + q] = lp[q];
        block_sync();
    }
    auto line = [&](int j, double out[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (STAGED) out[q] = slp[4 * (size_t)j + q];
            else out[q] = lp[4 * (size_t)j + q];
        }
    };
    const int grp = tid() / ROWG, gl = tid() % ROWG;
    const int i = blk * rpb + grp;
    const bool valid = i < N;
    const int ii = valid ? i : 0;
    double a[4];
    line(ii, a);
    if (A.lscore) {
        const int k1 = N < A.k1 ? N : A.k1;                     // :40-41
        const int k2 = N < A.k2 ? N : A.k2;
        double* ks = lds + grp * LR_KS;
        const LineGeom ga = line_geom(a);
        double td[LR_K];
        int tj[LR_K];
#pragma unroll
        for (int q = 0; q < LR_K; ++q) { td[q] = 1e300; tj[q] = 0x7fffffff; }
        for (int j0 = gl; j0 < N; j0 += 2 * ROWG) {             // two independent pairs per trip
            double dv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = j0 + u * ROWG;
                const int jj = j < N ? j : ii;
                double b[4];
                line(jj, b);
                const LineGeom gb = line_geom(b);
                const bool up = jj > ii;                        // a = the line of the larger index (see above)
                LineGeom p, s;
                p.x1 = up ? gb.x1 : ga.x1; p.y1 = up ? gb.y1 : ga.y1; p.x2 = up ? gb.x2 : ga.x2; p.y2 = up ? gb.y2 : ga.y2;
                p.dx = up ? gb.dx : ga.dx; p.dy = up ? gb.dy : ga.dy; p.nn = up ? gb.nn : ga.nn;
                s.x1 = up ? ga.x1 : gb.x1; s.y1 = up ? ga.y1 : gb.y1; s.x2 = up ? ga.x2 : gb.x2; s.y2 = up ? ga.y2 : gb.y2;
                s.dx = up ? ga.dx : gb.dx; s.dy = up ? ga.dy : gb.dy; s.nn = up ? ga.nn : gb.nn;
                const double d = line_distance_closest(p, s);
                dv[u] = j < N ? (j == ii ? 4.0 : d) : 1e300;    // :82
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                double nd = dv[u];
                int nj = (j0 + u * ROWG < N) ? j0 + u * ROWG : 0x7fffffff;
#pragma unroll
                for (int q = 0; q < LR_K; ++q) {
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
                for (int q = 0; q + 1 < LR_K; ++q) { td[q] = td[q + 1]; tj[q] = tj[q + 1]; }
                td[LR_K - 1] = 1e300;
                tj[LR_K - 1] = 0x7fffffff;
            }
            if (gl == 0) { ks[r] = (double)bj; ks[LR_K + r] = bd; }
        }
        wave_sync();
        const double len_a = norm2(a[0] - a[2], a[1] - a[3]);
        for (int q = gl; q < k1; q += ROWG) {
            int j = (int)ks[q];
            j = (valid && j >= 0 && j < N) ? j : 0;
            double b[4];
            line(j, b);
            ks[2 * LR_K + q] = lines_cosangle(a, b, 9.0);                          // :55
            // :65 lines_proximity measures the pair again: for the line itself (one of the k1 when N <= k1) that is
            // its distance from itself, 0 (NaN for a segment without length), not the 4 of the sorted row (:82)
            const double dq = j == ii ? line_distance_closest(a, b) : ks[LR_K + q];
            ks[3 * LR_K + q] = proximity(dq, len_a, line_length(b), A.sigma);
        }
        wave_sync();
        // np.argsort(cosphi)[::-1][0:k2] (:57-59): descending, ties -> later position first
        for (int q = gl; q < k1; q += ROWG) {
            const double cq = ks[2 * LR_K + q];
            int rank = 0;
            for (int p = 0; p < k1; ++p) {
                const double cp = ks[2 * LR_K + p];
                rank += (cp > cq) || (cp == cq && p > q);
            }
            if (rank < k2) ks[4 * LR_K + rank] = ks[3 * LR_K + q] * cq;                 // :66
        }
        wave_sync();
        if (gl == 0 && valid) {
            double sum = 0.0;
            for (int r = 0; r < k2; ++r) sum += ks[4 * LR_K + r];                       // :68, in rank order
            A.lscore[o0 + i] = sum / k2;                                            // :70
        }
    }
    if (gl == 0 && valid) {
        if (A.langle) A.langle[o0 + i] = line_angle(a);
        if (A.llen) A.llen[o0 + i] = line_length(a);
    }
}

// LDS of a rating workgroup in doubles: the groups' scratch and, for the images that are staged, 4 lds_lines doubles of lp
VPK_DEV void line_rating_block(const LineBatchArgs& A, int img, int blk) {
    const int N = uniform_int((int)(A.offsets[img + 1] - A.offsets[img]));
    if (N <= A.lds_lines) line_rating_rows<true>(A, img, blk);
    else line_rating_rows<false>(A, img, blk);
}

}  // namespace vpk
#endif
