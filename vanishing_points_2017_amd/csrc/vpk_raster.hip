// vpk_raster.hip -- the reference's sphere rasteriser (sphere_mapping.py:36-72) for gfx950, faithful to what the reference
// actually executes: matplotlib's Agg backend.
//
// The reference plots, for every line (a, b, c), beta(alpha) = atan((-a sin alpha - c cos alpha) / b) at 10 000 alpha in
// [-pi/2, pi/2] (:40,:61-63) with ax.plot(..., c=[1, 1, 1, alpha]) on black axes that fill a size x size canvas, reads the
// canvas back and averages R, G, B (:65-68).  What that does to a pixel is defined by third-party code -- matplotlib's
// RendererAgg::draw_path and the Anti-Grain Geometry library it embeds -- whose stages for a solid anti-aliased Line2D
// are restated here one by one (the CPU restatement, pinned bit for bit against matplotlib itself and against the
// rasters stored in tests/golden, is oracle/agg_raster.py; it cites the sources stage by stage):
//
//   curve -> pixels           x = (alpha + pi/2) / pi * W,  y = H - (beta + pi/2) / pi * H
//   PathSimplifier            runs of segments that stay within 1/9 px of the run's first segment's line are merged
//   agg::conv_stroke          width 100/72 px, projecting caps, round joins (mitred when almost straight), inner miter
//   rasterizer_scanline_aa    24.8 fixed-point cells (cover, area) with the canvas as clip box, non-zero winding
//   fixed_blender_rgba_plain  white, alpha8 = uround(255 alpha); per pixel a = round(alpha8 cover / 255);
//                             p' = ((65280 - 255 p) a + 65280 p) / (65280 + a), truncated; ONE LINE AFTER THE OTHER
//   the axes' four spines     0.8 pt black strokes snapped to the pixel centres of the border, drawn over the lines
//
// Five kernels, per chunk of images (the first once per canvas size):
//   raster_table_kernel  one THREAD per sample: pixel x, sin and cos of alpha, the same for every line (raster_curve.hpp)
//   simplify_kernel      one WAVE per line, lanes = samples: samples -> PathSimplifier's kept points (see the kernel)
//   outline_kernel       one THREAD per line: conv_stroke on the kept points (and the sequential simplifier for the lines
//                        simplify_kernel leaves to it); the closed outline polygons (up to MAXSUB per line) go to HBM
//   coverage_kernel      one WORKGROUP per line at a time (persistent workgroups over a queue of ALL lines: the lines of an
//                        image need no order here): cells in the LDS pool, sweep -> the line's coverage as one byte per
//                        pixel of every touched row's cell range (the pool's packing) + the dense row table, in HBM
//                        (raster_coverage.hpp: polygon_coverage, which the CPU suite runs too)
//   blend_kernel         32 image rows x 8 column segments per workgroup, the rows' pixels in LDS: the image's lines IN
//                        INPUT ORDER (the 8-bit blend does not commute), then the four spines; one coalesced store
#include "vpk_internal.hpp"
#include "raster_coverage.hpp"
#include "raster_curve.hpp"

#include <algorithm>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

namespace {

using namespace vpk_raster;

constexpr int POLY_INTS = 1 + 3 * MAXSUB;                // per line: sub-paths, then (first vertex, vertices, split column) each

// (passed to the kernels BY VALUE: the fields arrive in scalar registers, not behind a pointer)
struct RasterArgs {
    const double* l; const long long* offsets; const int* order; const double* tab;
    int batch; int size; int samples; unsigned a8; long long nlines; long long line0;   // this chunk: lines [line0, line0 + nlines)
    unsigned char* out; int* ctr; unsigned* flags;       // ctr[0]: coverage_kernel's line queue, ctr[8 .. 11]: the probe's laps
    unsigned long long* bump;                            // alpha bytes used
    V2* simp; V2* verts; int* polys;                     // per line: MAXS, MAXV, POLY_INTS
    int pool, rowcap;                                    // coverage_kernel: pool entries and row-array length in (dynamic) LDS
    int probe;                                           // VPK_RASTER_TIMES: workgroup 0 of coverage_kernel times its phases
    int* seq; int* nsimp; int force_seq;                 // per line: 1 = left to the sequential machine; points kept by simplify_kernel
    unsigned char* alpha; unsigned long long alpha_cap;
    RowEnt* dense;                                       // [nlines + 4 spines][MAXSUB][size]
    int first_image;                                     // images [first_image, first_image + batch) of the caller's batch
    int alt;                                             // 1: the reference's `alternative` curve (sphere_mapping.py:58-59)
};

// which image of the chunk line `gl` (of the caller's batch) belongs to: binary search in the offsets
__device__ __forceinline__ int image_of_line(const RasterArgs& A, long long gl) {
    int lo = 0, hi = A.batch;
    while (hi - lo > 1) { const int mid = (lo + hi) / 2; if (A.offsets[A.first_image + mid] <= gl) lo = mid; else hi = mid; }
    return lo;
}

__global__ void raster_table_kernel(int ns, int size, double* tab) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    curve_sample(i, ns, size, tab + 4 * i);
    tab[4 * i + 3] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------
// simplify_kernel: samples -> PathSimplifier with one WAVE per line, lanes = 64 consecutive samples.
//
// The simplifier is a sequential machine, but its state only changes shape when a run ends (about 60 times in 10 000
// samples); in between, what a vertex contributes -- its distance across and along the run -- depends on the run's
// constants alone.  So a wave evaluates 64 samples at once (the curve's beta(alpha), the axes' transform, the
// simplifier's metrics), finds the first lane that ends the run (ballot), folds the lanes before it into the state
// with two max-reductions (the farthest vertex forwards / backwards: strict `>` in sequence = the FIRST lane that
// attains the maximum, if that beats the incoming one; the two `last_*` flags = whether the last folded lane is that
// lane), performs the run's end in wave-uniform code, and goes on with the remaining lanes under the new run's constants.
// Same operations on the same operands as the vertex-by-vertex machine (raster_device.hpp: Simplifier), so the same
// points.  A line with a non-finite sample (b = 0 and friends: PathNanRemover breaks the path there) is left to the
// sequential machine in outline_kernel (seq[g] = 1).
// ---------------------------------------------------------------------------------------------------------------
using vpk::readlane_f64;                                 // (the lane: wave-uniform)
using vpk::uniform_int;
// (not vpk::wave_max: that one propagates NaN through nanmax -- two more compares and selects per step; no NaN gets here)
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}

__global__ __launch_bounds__(64) void simplify_kernel(RasterArgs A) {
    const long long g = blockIdx.x;
    const int lane = threadIdx.x;
    const long long gl = A.line0 + g;
    const double la = A.l[3 * gl], lb = A.l[3 * gl + 1], lc = A.l[3 * gl + 2];
    const int size = A.size, ns = A.samples;
    V2* out = A.simp + (size_t)g * MAXS;
    if (A.force_seq) { if (lane == 0) A.seq[g] = 1; return; }
    // the machine's state (every lane holds the same values)
    const double thr2 = (1.0 / 9.0) * (1.0 / 9.0);
    double lastx = 0, lasty = 0, origdx = 0, origdy = 0, orig_norm2 = 0, fwd_max = 0, bwd_max = 0, nextx = 0, nexty = 0, nbx = 0,
           nby = 0, startx = 0, starty = 0;
    bool last_fwd = false, last_bwd = false, clipped = true, started = false;
    int n = 0, overflow = 0;
    auto emit = [&](double x, double y) {
        if (n < MAXS) { if (lane == 0) { out[n].x = x; out[n].y = y; } ++n; } else overflow = 1;
    };
    for (int c0 = 0; c0 < ns; c0 += 64) {
        const int i = c0 + lane;
        const bool valid = i < ns;
        const int ic = valid ? i : ns - 1;
        const double sa = A.tab[4 * ic + 1], ca = A.tab[4 * ic + 2], x = A.tab[4 * ic];
        const double y = curve_y(curve_beta(la, lb, lc, sa, ca, A.alt), size);
        const unsigned long long bad = __ballot(valid && (!(y == y) || isinf(y)));
        unsigned long long pending = __ballot(valid);
        if (bad != 0ull) {
            // PathNanRemover's business.  A line whose samples are ALL non-finite (the all-zero line: 0 / 0 everywhere)
            // draws nothing and is settled here; any other mixture goes to the sequential machine.
            if (bad == pending && !started) continue;
            if (lane == 0) A.seq[g] = 1;
            return;
        }
        if (!started) {                                                       // move_to (the first finite sample)
            if (c0 != 0) { if (lane == 0) A.seq[g] = 1; return; }             // (finite samples after non-finite ones: a broken path)
            lastx = readlane_f64(x, 0); lasty = readlane_f64(y, 0);
            orig_norm2 = 0.0; bwd_max = 0.0; clipped = true; started = true;
            pending &= ~1ull;
        }
        while (pending != 0ull) {
            if (uniform_int(orig_norm2 == 0.0)) {                             // the run's first segment
                const int j = uniform_int(__builtin_ctzll(pending));
                const double px = readlane_f64(x, j), py = readlane_f64(y, j);
                if (clipped) { emit(lastx, lasty); clipped = false; }
                origdx = px - lastx; origdy = py - lasty;
                orig_norm2 = origdx * origdx + origdy * origdy;
                fwd_max = orig_norm2; bwd_max = 0.0; last_fwd = true; last_bwd = false;
                startx = lastx; starty = lasty;
                nextx = lastx = px; nexty = lasty = py;
                pending &= ~(1ull << j);
                continue;
            }
            // metrics of every lane's vertex under the run's constants (Simplifier::metrics)
            const double totdx = x - startx, totdy = y - starty;
            const double totdot = origdx * totdx + origdy * totdy;
            const double paradx = totdot * origdx / orig_norm2, parady = totdot * origdy / orig_norm2;
            const double perpdx = totdx - paradx, perpdy = totdy - parady;
            const double perp2 = perpdx * perpdx + perpdy * perpdy;
            const double para2 = paradx * paradx + parady * parady;
            const bool mine = (pending >> lane) & 1ull;
            const unsigned long long brk = __ballot(mine && !(perp2 < thr2));
            const int jb = brk ? uniform_int(__builtin_ctzll(brk)) : 64;
            const unsigned long long inrun = jb < 64 ? (pending & ((1ull << jb) - 1ull)) : pending;
            if (inrun != 0ull) {
                const bool in = (inrun >> lane) & 1ull;
                const int jl = uniform_int(63 - __builtin_clzll(inrun));      // the last vertex folded in
                const bool fwd_el = in && totdot > 0.0, bwd_el = in && !(totdot > 0.0);
                bool lf = false, lbk = false;
                // (a curve usually runs on along its run: the last folded lane is the farthest one forwards, and one ballot
                //  says so -- "no eligible lane reaches its para2" -- without the reduction)
                const double pl = readlane_f64(para2, jl);
                const bool jl_fwd = (__ballot(fwd_el) >> jl) & 1ull;
                if (jl_fwd && __ballot(fwd_el && para2 >= pl) == (1ull << jl)) {
                    if (uniform_int(pl > fwd_max)) { fwd_max = pl; nextx = readlane_f64(x, jl); nexty = readlane_f64(y, jl); lf = true; }
                } else if (__ballot(fwd_el) != 0ull) {
                    const double m = wave_max(fwd_el ? para2 : -1.0);
                    if (uniform_int(m > fwd_max)) {
                        const int jf = uniform_int(__builtin_ctzll(__ballot(fwd_el && para2 == m)));
                        fwd_max = m; nextx = readlane_f64(x, jf); nexty = readlane_f64(y, jf);
                        lf = jf == jl;
                    }
                }
                if (__ballot(bwd_el) != 0ull) {
                    const double m = wave_max(bwd_el ? para2 : -1.0);
                    if (uniform_int(m > bwd_max)) {
                        const int jk = uniform_int(__builtin_ctzll(__ballot(bwd_el && para2 == m)));
                        bwd_max = m; nbx = readlane_f64(x, jk); nby = readlane_f64(y, jk);
                        lbk = jk == jl;
                    }
                }
                last_fwd = lf; last_bwd = lbk;
                lastx = readlane_f64(x, jl); lasty = readlane_f64(y, jl);
            }
            if (jb < 64) {                                                    // _push: the run ends at lane jb's vertex
                const double px = readlane_f64(x, jb), py = readlane_f64(y, jb);
                const bool both = bwd_max > 0.0;
                const double ax = both && last_fwd ? nbx : nextx, ay = both && last_fwd ? nby : nexty;
                const double cx = last_fwd ? nextx : nbx, cy = last_fwd ? nexty : nby;
                emit(ax, ay);
                if (both) emit(cx, cy);
                double ex = both ? cx : ax, ey = both ? cy : ay;
                if (clipped || (!last_fwd && !last_bwd)) { emit(lastx, lasty); ex = lastx; ey = lasty; }
                origdx = px - lastx; origdy = py - lasty;
                orig_norm2 = origdx * origdx + origdy * origdy;
                fwd_max = orig_norm2; last_fwd = true;
                startx = ex; starty = ey;
                lastx = nextx = px; lasty = nexty = py;
                bwd_max = 0.0; last_bwd = false; clipped = false;
                pending &= ~((2ull << jb) - 1ull);
            } else {
                pending = 0ull;
            }
        }
    }
    // path_cmd_stop
    if (started) {
        if (orig_norm2 != 0.0) {
            emit(nextx, nexty);
            if (bwd_max > 0.0) emit(nbx, nby);
        }
        emit(lastx, lasty);
    }
    if (lane == 0) { A.seq[g] = 0; A.nsimp[g] = n | (overflow ? 0x40000000 : 0); }
}

__global__ __launch_bounds__(64) void outline_kernel(RasterArgs A) {
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;     // line of this chunk; the 4 spines follow the lines
    if (g >= A.nlines + 4) return;
    V2* sp = A.simp + (size_t)g * MAXS;
    Outline o;
    unsigned dummy = 0;
    unsigned* fl = &dummy;
    o.v = A.verts + (size_t)g * MAXV; o.n = 0; o.cap = MAXV; o.flags = fl;
    int* pt = A.polys + g * POLY_INTS;
    const int size = A.size;
    if (g >= A.nlines) {
        spine_path((int)(g - A.nlines), size, sp);
        stroke_outline(sp, 2, SPINE_WIDTH_PX, o);
        pt[0] = 1; pt[1] = 0; pt[2] = o.n; pt[3] = size + 2;        // (a spine: one range per row)
        return;
    }
    const double width_px = LINE_WIDTH_PX;
    const long long gl = A.line0 + g;
    int npoly = 0;
    Simplifier sm;
    sm.init(sp, MAXS);
    const int ns = A.samples;
    auto flush = [&]() {                                  // end of a sub-path: stroke what the simplifier kept
        sm.end();
        if (sm.n >= 2) {
            const int first = o.n;
            const int xsp = split_column(sp, sm.n, size);
            stroke_outline(sp, sm.n, width_px, o);
            if (o.n - first >= 3) {
                if (npoly < MAXSUB) { pt[1 + 3 * npoly] = first; pt[2 + 3 * npoly] = o.n - first; pt[3 + 3 * npoly] = xsp; ++npoly; }
                else dummy |= FLAG_OVERFLOW;
            }
        }
        sm.n = 0;
    };
    if (A.seq[g]) {
        // the sequential machine (lines with non-finite samples; VPK_RASTER_SEQUENTIAL=1: every line): SAMPLE_GROUP samples
        // are evaluated side by side (independent division / atan chains), then fed to the simplifier as a group
        const double la = A.l[3 * gl], lb = A.l[3 * gl + 1], lc = A.l[3 * gl + 2];
        constexpr int OG = SAMPLE_GROUP;
        for (int i0 = 0; i0 < ns; i0 += OG) {
            double xs[OG], ys[OG];
#pragma unroll
            for (int u = 0; u < OG; ++u) {
                const int i = i0 + u < ns ? i0 + u : ns - 1;
                const double sa = A.tab[4 * i + 1], ca = A.tab[4 * i + 2];
                const double be = curve_beta(la, lb, lc, sa, ca, A.alt);
                xs[u] = A.tab[4 * i];
                ys[u] = curve_y(be, size);
            }
            feed_group<OG>(sm, xs, ys, ns - i0, flush);
        }
    } else {
        // simplify_kernel kept the line's points: one finished path
        const int k = A.nsimp[g];
        sm.n = k & 0xffff;
        if (k & 0x40000000) dummy |= FLAG_OVERFLOW;
        sm.have = false;
        if (sm.n >= 2) {
            const int xsp = split_column(sp, sm.n, size);
            stroke_outline(sp, sm.n, width_px, o);
            if (o.n >= 3) { pt[1] = 0; pt[2] = o.n; pt[3] = xsp; npoly = 1; }
        }
        sm.n = 0;
    }
    if (sm.have) flush();
    pt[0] = npoly;
    dummy |= sm.overflow;
    if (dummy) atomicOr(A.flags + A.first_image + image_of_line(A, gl), dummy);
}

__global__ __launch_bounds__(RT, 3) void coverage_kernel(RasterArgs A) {   // three workgroups (of four waves) per CU
    extern __shared__ int s_dyn[];                       // six row arrays of A.rowcap ints, then the pool (cover, area)
    __shared__ __attribute__((aligned(16))) CovShared S; // (16: a vertex is stored as one 128-bit LDS write)
    const int size = A.size, rc = A.rowcap;
    int* s_rowmin = s_dyn; int* s_rowmax = s_dyn + rc; int* s_rowoff = s_dyn + 2 * rc;
    int* s_rmin = s_dyn + 3 * rc; int* s_rmax = s_dyn + 4 * rc; int* s_lcov = s_dyn + 5 * rc;
    int* s_pcover = s_dyn + 6 * rc; int* s_parea = s_pcover + A.pool;
    CellSink sink;
    sink.rowmin = (lds_int_ptr)s_rowmin; sink.rowmax = (lds_int_ptr)s_rowmax; sink.rowoff = (lds_int_ptr)s_rowoff; sink.size = size;
    sink.rmin = (lds_int_ptr)s_rmin; sink.rmax = (lds_int_ptr)s_rmax; sink.lcov = (lds_int_ptr)s_lcov; sink.xs = 0;
    sink.pcover = (lds_int_ptr)s_pcover; sink.parea = (lds_int_ptr)s_parea;
    sink.blo = 0; sink.bhi = 0; sink.boff = 0;
    CovOut O;
    O.alpha = A.alpha; O.alpha_cap = A.alpha_cap; O.bump = A.bump; O.pool = A.pool; O.probe = A.probe; O.laps = A.ctr + 8;
    for (int y = threadIdx.x; y < rc; y += RT) {
        s_rowmin[y] = 0x7fffffff; s_rowmax[y] = -1; s_rowoff[y] = 0; s_rmin[y] = 0x7fffffff; s_rmax[y] = -1; s_lcov[y] = 0;
    }
    for (int q = threadIdx.x; q < A.pool; q += RT) { s_pcover[q] = 0; s_parea[q] = 0; }   // the sweeps leave the pool zero again
    if (threadIdx.x == 0) S.next = atomicAdd(A.ctr, 1);
    __syncthreads();
    for (;;) {
        const long long g = __builtin_amdgcn_readfirstlane(S.next);
        __syncthreads();
        if (g >= A.nlines + 4) break;
        int nx = 0;
        if (threadIdx.x == 0) nx = atomicAdd(A.ctr, 1);  // the line after this one: the round trip runs beside the work below
        const int* pt = A.polys + g * POLY_INTS;
        const int npoly = pt[0];
        const int more = (npoly > 1 ? npoly - 1 : 0) << ROW_MORE_SHIFT;
        for (int q = 0; q < (npoly > 0 ? npoly : 1); ++q) {
            RowEnt* ent = A.dense + ((size_t)g * MAXSUB + q) * size;
            if (q < npoly) {
                const bool ok = polygon_coverage(A.verts + (size_t)g * MAXV + pt[1 + 3 * q], pt[2 + 3 * q], pt[3 + 3 * q], sink, size, S,
                                                 O, ent, q == 0 ? more : 0);
                if (!ok && threadIdx.x == 0 && g < A.nlines)                        // dropped: tell the line's image
                    atomicOr(A.flags + A.first_image + image_of_line(A, A.line0 + g), FLAG_OVERFLOW);
            } else {                                      // a line that left no polygon: an empty sub-path 0
                for (int y = threadIdx.x; y < size; y += RT) ent[y] = untouched_row(0);
            }
        }
        if (threadIdx.x == 0) S.next = nx;
        __syncthreads();
    }
}

// The blend.  sweep_scanline + render_scanline_aa_solid per pixel: an entry of a row's cell range with area got
// calculate_alpha((R << 9) - area), one without (no cell, or a cell of a vertical edge on the pixel boundary) lies in the
// span that runs to the next cell and got calculate_alpha(R << 9) -- 0 after the row's last cell --, R = running cover;
// coverage_kernel stored those alphas.  Here: fixed_blender_rgba_plain, item after item.
constexpr int BROWS = 32, BSEG = 8;                       // image rows per workgroup x column segments per row: 256 threads
                                                         // (measured, 102 / 95 images: 8 x 8 0.66 / 1.59 ms, 16 x 8 0.77 / 1.47,
                                                         //  32 x 8 0.74 / 1.37)
constexpr unsigned BLEND_LUT_MAX_A8 = 63;                // colour alphas up to this blend through a table (17 KB of LDS at most)
// blend_kernel's dynamic LDS: the rows' pixels, amul, and the tables of a colour alpha a8 (none beyond BLEND_LUT_MAX_A8)
constexpr size_t blend_lds(int size, unsigned a8) {
    return (size_t)BROWS * ((size + 3) & ~3) + 256 + (a8 <= BLEND_LUT_MAX_A8 ? (size_t)(a8 + 1) * 256 : 0);
}
__global__ __launch_bounds__(BROWS * BSEG) void blend_kernel(RasterArgs A) {
    extern __shared__ unsigned char s_px[];              // [BROWS][size rounded to 4], then the tables
    const int size = A.size, ldp = (size + 3) & ~3;
    const int rr = threadIdx.x & (BROWS - 1), seg = threadIdx.x / BROWS;
    const int img_i = A.order[A.first_image + blockIdx.y], y = blockIdx.x * BROWS + rr;   // images with many lines first
    unsigned char* row = s_px + (size_t)rr * ldp;
    // The blend of a white line is a function of (pixel, cover) with few distinct colour alphas (26 * cover / 255 = 0..26
    // at the reference's alpha 0.1): two table reads instead of the blender's multiplications and its division --
    //   amul[cover] = multiply(a8, cover),   lut[alpha][pixel] = fixed_blender_rgba_plain(pixel, white, alpha)
    unsigned char* amul = s_px + (size_t)BROWS * ldp;
    unsigned char* lut = amul + 256;
    const bool tables = A.a8 <= BLEND_LUT_MAX_A8;
    if (tables) {
        for (int q = threadIdx.x; q < 256; q += BROWS * BSEG) amul[q] = (unsigned char)cover_alpha(A.a8, (unsigned)q);
        for (int q = threadIdx.x; q < (int)(A.a8 + 1) * 256; q += BROWS * BSEG)
            lut[q] = (unsigned char)blend_alpha((unsigned)q & 255u, 255u, (unsigned)q >> 8);
    }
    // a thread owns the pixels [x0, x1) of its row: rows with long cell ranges (curves running along the row) are shared
    // by the waves, and a workgroup keeps them all in flight against the latency of the item -> row -> alpha loads
    const int segw = ((size + BSEG - 1) / BSEG + 3) & ~3;
    const int x0 = seg * segw, x1 = x0 + segw < size ? x0 + segw : size;
    for (int x = x0; x < x0 + segw && x < ldp; x += 4) *reinterpret_cast<unsigned*>(row + x) = 0u;
    const long long lo = A.offsets[A.first_image + img_i] - A.line0, hi = A.offsets[A.first_image + img_i + 1] - A.line0;
    __syncthreads();
    if (y < size) {
        const RowEnt* dl = A.dense + y;                   // this row's entries: dl[(line * MAXSUB + sub-path) * size]
        // eight consecutive pixels.  Through the tables every step is eight independent LDS reads (old pixels, colour alphas,
        // new pixels: alpha 0 maps a pixel to itself), then the writes -- of the pixels with coverage only: a thread must not
        // touch its neighbours' columns, not even to write back what it read.  (Eight `if (cover) pixel = ...` in a row
        // are eight dependent read chains.)  use_tables: std::true_type / std::false_type, a compile-time choice in here.
        auto blend8 = [&](const unsigned (&av)[8], int xbase, unsigned grey, unsigned a8, auto use_tables) {
            if constexpr (decltype(use_tables)::value) {
                unsigned old[8], ca[8], nv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { old[u] = row[xbase + u]; ca[u] = amul[av[u]]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) nv[u] = lut[(ca[u] << 8) | old[u]];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (av[u]) row[xbase + u] = (unsigned char)nv[u];
            } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int x = xbase + u;
                    if (av[u]) row[x] = (unsigned char)blend(row[x], grey, a8, av[u]);
                }
            }
        };
        auto seg_range = [&](const Range& r, int& qlo, int& qhi) {    // the range's bytes that fall into this thread's columns
            qlo = x0 - r.xmin > 0 ? x0 - r.xmin : 0;
            qhi = x1 - r.xmin < r.len ? x1 - r.xmin : r.len;
        };
        // Eight alpha bytes are ONE unaligned 8-byte load (the hardware takes unaligned global addresses; up to seven bytes
        // past the range's end are read and masked away: the pool has slack behind it).  Loads are issued unconditionally
        // -- an empty range reads the pool's first bytes -- so that the compiler can COUNT the loads in flight: a skipped
        // load makes every later wait a wait for everything.
        typedef unsigned long long __attribute__((aligned(1))) u64u;
        auto fetch8 = [&](const Range& r, int q0, int qhi) {
            return *reinterpret_cast<const u64u*>(A.alpha + (q0 < qhi ? (size_t)r.off + q0 : 0));
        };
        auto unpack8 = [&](unsigned long long w, int q0, int qhi, unsigned (&av)[8]) {
#pragma unroll
            for (int u = 0; u < 8; ++u) av[u] = q0 + u < qhi ? (unsigned)(w >> (8 * u)) & 255u : 0u;
        };
        auto rest = [&](const Range& r, int qlo, int qhi, unsigned grey, unsigned a8, auto use_tables) {   // bytes past the first eight
            for (int q0 = qlo + 8; q0 < qhi; q0 += 8) {
                unsigned av[8];
                unpack8(fetch8(r, q0, qhi), q0, qhi, av);
                blend8(av, r.xmin + q0, grey, a8, use_tables);
            }
        };
        auto whole = [&](const Range& r, unsigned grey, unsigned a8, auto use_tables) {
            int qlo, qhi;
            seg_range(r, qlo, qhi);
            if (qlo < qhi) {
                unsigned av[8];
                unpack8(fetch8(r, qlo, qhi), qlo, qhi, av);
                blend8(av, r.xmin + qlo, grey, a8, use_tables);
                rest(r, qlo, qhi, grey, a8, use_tables);
            }
        };
        // the lines' colour alpha blends through the tables or not: decided here, once per call site, and handed on as the
        // last argument (std::true_type / std::false_type)
        auto with_tables = [&](auto&& f, auto&&... a) { if (tables) f(a..., std::true_type()); else f(a..., std::false_type()); };
        auto line_range = [&](const unsigned (&av)[8], const Range& r, int qlo, int qhi, auto t) {     // av: its first eight bytes
            blend8(av, r.xmin + qlo, 255u, A.a8, t); rest(r, qlo, qhi, 255u, A.a8, t);
        };
        auto line_entry = [&](const RowEnt& f, auto t) { whole(range_l(f), 255u, A.a8, t); whole(range_r(f), 255u, A.a8, t); };
        // The image's lines in order -- the blend does not commute -- but FETCHED ahead: the dense table needs no knowledge
        // about a line to address its entry, so while group k (BL lines, two ranges each) is blended (LDS), the first eight
        // alpha bytes of group k + 1's ranges and the entries of group k + 2 are in flight.
        constexpr int BL = 2, NR = 2 * BL;
        const long long last = hi - 1;
        const RowEnt none = {0u, 0, 0, 0, 0, 0};
        auto entries = [&](long long g0, RowEnt (&e)[BL]) {
#pragma unroll
            for (int u = 0; u < BL; ++u) {
                const long long g = g0 + u < hi ? g0 + u : (last > lo ? last : lo);     // (clamped: masked below)
                e[u] = dl[(size_t)g * MAXSUB * size];
            }
        };
        auto settle = [&](long long g0, RowEnt (&e)[BL]) {
#pragma unroll
            for (int u = 0; u < BL; ++u) if (!(g0 + u < hi)) e[u] = none;
        };
        auto ranges_of = [&](const RowEnt (&e)[BL], Range (&r)[NR]) {
#pragma unroll
            for (int u = 0; u < BL; ++u) { r[2 * u] = range_l(e[u]); r[2 * u + 1] = range_r(e[u]); }
        };
        RowEnt e0[BL], e1[BL], e2[BL];
        Range r0[NR], r1[NR];
        unsigned long long w0[NR], w1[NR];
        int ql0[NR], qh0[NR], ql1[NR], qh1[NR];
        if (lo < hi) {
            entries(lo, e0); entries(lo + BL, e1);
            settle(lo, e0);
            ranges_of(e0, r0);
#pragma unroll
            for (int u = 0; u < NR; ++u) { seg_range(r0[u], ql0[u], qh0[u]); w0[u] = fetch8(r0[u], ql0[u], qh0[u]); }
        }
        for (long long g0 = lo; g0 < hi; g0 += BL) {
            entries(g0 + 2 * BL, e2);
            settle(g0 + BL, e1);
            ranges_of(e1, r1);
#pragma unroll
            for (int u = 0; u < NR; ++u) { seg_range(r1[u], ql1[u], qh1[u]); w1[u] = fetch8(r1[u], ql1[u], qh1[u]); }
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                if (ql0[u] < qh0[u]) {
                    unsigned av[8];
                    unpack8(w0[u], ql0[u], qh0[u], av);
                    with_tables(line_range, av, r0[u], ql0[u], qh0[u]);
                }
                if (u & 1) {                              // after a line's second range: its further sub-paths (rare)
                    const int more = (e0[u >> 1].lenL >> ROW_MORE_SHIFT) & 7;
                    for (int q = 1; q <= more; ++q) {
                        const RowEnt f = dl[((size_t)(g0 + (u >> 1)) * MAXSUB + q) * size];
                        with_tables(line_entry, f);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < BL; ++u) { e0[u] = e1[u]; e1[u] = e2[u]; }
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                r0[u] = r1[u]; ql0[u] = ql1[u]; qh0[u] = qh1[u]; w0[u] = w1[u];
            }
        }
        for (int side = 0; side < 4; ++side) {
            const RowEnt f = dl[(size_t)(A.nlines + side) * MAXSUB * size];
            whole(range_l(f), 0u, 255u, std::false_type());
            whole(range_r(f), 0u, 255u, std::false_type());
        }
    }
    __syncthreads();
    // coalesced store of the workgroup's rows
    unsigned char* out = A.out + (size_t)(A.first_image + img_i) * size * size;
    const int row0 = blockIdx.x * BROWS;
    for (int r = 0; r < BROWS && row0 + r < size; ++r)
        for (int x = threadIdx.x; x < size; x += BROWS * BSEG) out[(size_t)(row0 + r) * size + x] = s_px[(size_t)r * ldp + x];
}

// ---------------------------------------------------------------------------------------------------------------
// the host side
// ---------------------------------------------------------------------------------------------------------------
// The call's workspace (h->raster_hdr) as byte offsets.  The head -- everything up to `table` -- depends on the batch alone:
// vpk_sphere_raster_flags finds the flags of the last call from its batch.
struct RasterLayout {
    size_t offsets, order;                               // [batch + 1] line offsets (64 bit), [batch] the blend's image order
    size_t ctr, bump, flags;                             // per chunk (cleared for each): coverage_kernel's line queue and the
                                                         // probe's laps, the alpha pool's bump counter; per image: the flags
    size_t table;                                        // [samples][4] doubles (raster_table_kernel)
    size_t seq, nsimp, simp, verts, polys;               // per line of the largest chunk and spine
    size_t alpha, alpha_bytes;                           // the coverage pool
    size_t dense;                                        // RowEnt [lines + 4][MAXSUB][size]
    size_t bytes;
};
RasterLayout raster_layout(int batch, long long chunk_lines, int size, int samples, bool alt) {
    RasterLayout L;
    size_t p = 0;
    auto take = [&](size_t bytes) { const size_t at = p; p += bytes; return at; };
    auto align = [&]() { p = vpk::em_align(p, 256); };
    L.offsets = take((size_t)(batch + 1) * 8); L.order = take((size_t)batch * 4); align();
    L.ctr = take(64); L.bump = take(192); L.flags = take((size_t)batch * 4); align();
    L.table = take((size_t)samples * 4 * 8); align();
    const size_t nl = (size_t)chunk_lines + 4;
    L.seq = take(nl * 4); align();
    L.nsimp = take(nl * 4); align();
    L.simp = take(nl * MAXS * sizeof(V2));
    L.verts = take(nl * MAXV * sizeof(V2));
    L.polys = take(nl * POLY_INTS * 4); align();
    // the coverage pool: 16 KB per line on average (measured: ~6 KB) and never less than eight canvases' worth -- the row
    // ranges of ONE line can span most of the canvas (see polygon_coverage), and a call may consist of one line.  (The
    // `alternative` curve has a pole: a row can be crossed three times -- left branch, the jump, right branch -- and a row
    // range then spans half the canvas, so its lines get a canvas' worth of coverage pool each.)
    L.alpha_bytes = std::max<size_t>(nl * (alt ? (size_t)size * (size + 2) : (size_t)16384), (size_t)8 * size * (size + 2));
    L.alpha = take(L.alpha_bytes); align();
    L.dense = take(nl * MAXSUB * size * sizeof(RowEnt));
    L.bytes = p + 8192;                                  // (slack: the blend's 8-byte reads run past the pool's last range)
    return L;
}

// images [b0, b1) of one chunk: as many whole images as stay within max_lines lines, one at least
int chunk_end(const int64_t* offsets, int b0, int batch, long long max_lines) {
    int b1 = b0 + 1;
    while (b1 < batch && offsets[b1 + 1] - offsets[b0] <= max_lines) ++b1;
    return b1;
}

// VPK_RASTER_TIMES (development): the device time of a chunk's kernels, printed to stderr.  Owns the events.
struct ChunkTimes {
    enum { START, SIMPLIFY, OUTLINE, COVERAGE, BLEND, MARKS };
    const bool on; hipStream_t stream; hipEvent_t ev[MARKS] = {};
    ChunkTimes(bool enabled, hipStream_t s) : on(enabled), stream(s) {}
    ~ChunkTimes() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t mark(int q) {
        if (!on) return hipSuccess;
        const hipError_t e = hipEventCreate(&ev[q]);
        return e != hipSuccess ? e : hipEventRecord(ev[q], stream);
    }
    hipError_t report(const RasterArgs& A) {
        if (!on) return hipSuccess;
        float ms[MARKS] = {};
        hipError_t e = hipEventSynchronize(ev[BLEND]);
        for (int q = SIMPLIFY; q < MARKS && e == hipSuccess; ++q) e = hipEventElapsedTime(&ms[q], ev[q - 1], ev[q]);
        unsigned long long bump = 0;
        int dbg[16];
        if (e == hipSuccess) e = hipMemcpy(&bump, A.bump, 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(dbg, A.ctr, sizeof(dbg), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        fprintf(stderr, "vpk_sphere_raster: %d images, %lld lines: simplify %.2f + outlines %.2f ms, coverage %.2f ms, blend %.2f ms; %.0f coverage bytes "
                "per line; workgroup 0 of the coverage kernel: bounds %.2f, scan %.2f, cells %.2f, sweep %.2f ms\n", A.batch,
                A.nlines, ms[SIMPLIFY], ms[OUTLINE], ms[COVERAGE], ms[BLEND], (double)bump / (A.nlines + 4), dbg[8] * 1e-5, dbg[9] * 1e-5,
                dbg[10] * 1e-5, dbg[11] * 1e-5);
        return hipSuccess;
    }
};

}  // namespace

extern "C" {

int vpk_sphere_raster(vpk_handle* h, const double* l, const int64_t* offsets, int batch, int size, double alpha,
                      uint8_t* out) {
    static_assert(MAX_SIZE == 1024, "the message below names the limit");
    if (!h || !offsets || !out || batch < 1 || size < 8 || size > MAX_SIZE || !(alpha >= 0.0 && alpha <= 1.0) ||
        (!l && offsets[batch] != offsets[0]))             // (no lines at all: the frame-only canvas, l may be NULL)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_sphere_raster: bad argument (size must be 8..1024, alpha 0..1)");
    VPK_HIP(h, hipSetDevice(h->device));
    for (int b = 0; b < batch; ++b)
        if (offsets[b + 1] < offsets[b]) return vpk_fail(h, VPK_ERR_ARG, "vpk_sphere_raster: offsets not monotone");
    const bool force_seq = getenv("VPK_RASTER_SEQUENTIAL") != nullptr;   // development / tests: every line through the sequential machine
    const bool times = getenv("VPK_RASTER_TIMES") != nullptr;            // development: per-kernel device time
    // images are processed in chunks of at most ~48k lines (workspace per line: outline scratch + coverage pools); in
    // `alternative` mode, whose lines get a canvas' worth of coverage pool each (raster_layout), in smaller ones
    const bool alt = h->raster_alternative != 0;
    const long long max_lines = alt ? std::max<long long>(1, std::min<long long>(49152, (3ll << 30) / ((long long)size * (size + 2)))) : 49152;
    long long chunk_lines = 0;
    for (int b0 = 0, b1; b0 < batch; b0 = b1) {           // the largest chunk decides the workspace
        b1 = chunk_end(offsets, b0, batch, max_lines);
        chunk_lines = std::max<long long>(chunk_lines, offsets[b1] - offsets[b0]);
    }
    const RasterLayout L = raster_layout(batch, chunk_lines, size, SAMPLES, alt);
    if (L.alpha_bytes >= (1ull << 32)) {                  // RowEnt::off is 32 bits (a chunk of 49 152 lines needs 0.8 GB)
        // one image is one chunk at least; the pool per line is 16 KB, or a whole canvas in `alternative` mode.  The largest
        // count that passes: (lines + 4) * per_line <= 2^32 - 1 (262 139 lines at 16 KB: 2^32 is a multiple of it)
        char msg[160];
        snprintf(msg, sizeof msg, "vpk_sphere_raster: one image has more than %lld lines (the 4 GiB coverage pool at %s per line)",
                 (long long)(((1ull << 32) - 1) / (alt ? (size_t)size * (size + 2) : (size_t)16384)) - 4,
                 alt ? "one canvas (alternative mode)" : "16 KB");
        return vpk_fail(h, VPK_ERR_LIMIT, msg);
    }
    const size_t had_bytes = h->raster_hdr_bytes;
    int rc = vpk_reserve(h, &h->raster_hdr, &h->raster_hdr_bytes, L.bytes, "hipMalloc(raster workspace)");
    if (rc) return rc;
    if (h->raster_hdr_bytes != had_bytes) {               // a fresh allocation (possibly at the old address): nothing cached in it
        h->raster_offsets.clear();
        h->raster_table_size = 0;
    }
    h->raster_last_batch = batch;
    char* base = (char*)h->raster_hdr;
    // offsets [host] -> device.  Caller-owned pageable memory, so the copy is waited for -- but a pipeline rasterises the
    // same batch structure again and again: when the device copy already holds these offsets nothing is uploaded and the
    // call does not wait for anything (the sample table is kept the same way).
    const bool same = h->raster_offsets.size() == (size_t)batch + 1 &&
                      memcmp(h->raster_offsets.data(), offsets, (size_t)(batch + 1) * 8) == 0;
    if (!same) {
        VPK_HIP(h, hipStreamSynchronize(h->stream));
        VPK_HIP(h, hipMemcpyAsync(base + L.offsets, offsets, (size_t)(batch + 1) * 8, hipMemcpyHostToDevice, h->stream));
        // the blend's workgroups of an image last as long as the image has lines: within a chunk the images are dealt out
        // longest first, so that the kernel does not end on a 400-line image that started last
        std::vector<int> order((size_t)batch);
        for (int b0 = 0, b1; b0 < batch; b0 = b1) {
            b1 = chunk_end(offsets, b0, batch, max_lines);
            for (int b = b0; b < b1; ++b) order[b] = b - b0;
            std::stable_sort(order.begin() + b0, order.begin() + b1, [&](int x, int y) {
                return offsets[b0 + x + 1] - offsets[b0 + x] > offsets[b0 + y + 1] - offsets[b0 + y]; });
        }
        VPK_HIP(h, hipMemcpyAsync(base + L.order, order.data(), (size_t)batch * 4, hipMemcpyHostToDevice, h->stream));
        VPK_HIP(h, hipStreamSynchronize(h->stream));
        h->raster_offsets.assign((const long long*)offsets, (const long long*)offsets + batch + 1);
    }
    VPK_HIP(h, hipMemsetAsync(base + L.ctr, 0, L.table - L.ctr, h->stream));
    if (!same || h->raster_table_size != size) {
        hipLaunchKernelGGL(raster_table_kernel, dim3((SAMPLES + 255) / 256), dim3(256), 0, h->stream, SAMPLES, size, (double*)(base + L.table));
        h->raster_table_size = size;
    }
    RasterArgs A;
    A.l = l; A.offsets = (const long long*)(base + L.offsets); A.order = (const int*)(base + L.order); A.tab = (const double*)(base + L.table);
    A.size = size; A.samples = SAMPLES;
    A.a8 = (unsigned)(alpha * 255.0 + 0.5);               // agg::rgba8(rgba): uround
    A.out = out; A.ctr = (int*)(base + L.ctr); A.bump = (unsigned long long*)(base + L.bump); A.flags = (unsigned*)(base + L.flags);
    A.seq = (int*)(base + L.seq); A.nsimp = (int*)(base + L.nsimp);
    A.force_seq = force_seq; A.probe = times ? 1 : 0;
    A.alt = h->raster_alternative;
    A.simp = (V2*)(base + L.simp); A.verts = (V2*)(base + L.verts); A.polys = (int*)(base + L.polys);
    A.alpha = (unsigned char*)(base + L.alpha); A.alpha_cap = L.alpha_bytes;
    A.dense = (RowEnt*)(base + L.dense);
    A.rowcap = coverage_rowcap(size);
    A.pool = coverage_pool(size);
    const size_t cov_dyn = (size_t)(6 * A.rowcap + 2 * A.pool) * 4;
    if (!h->raster_ready) {
        VPK_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(blend_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)blend_lds(MAX_SIZE, BLEND_LUT_MAX_A8)));
        VPK_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(coverage_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       COV_LDS - COV_STATIC));
        h->raster_ready = true;
    }
    for (int b0 = 0, b1; b0 < batch; b0 = b1) {
        b1 = chunk_end(offsets, b0, batch, max_lines);
        A.first_image = b0; A.batch = b1 - b0; A.line0 = offsets[b0]; A.nlines = offsets[b1] - offsets[b0];
        VPK_HIP(h, hipMemsetAsync(base + L.ctr, 0, L.flags - L.ctr, h->stream));    // queue + bump counters of this chunk
        const long long nt = A.nlines + 4;
        ChunkTimes t(times, h->stream);
        VPK_HIP(h, t.mark(ChunkTimes::START));
        if (A.nlines > 0)                                 // (a chunk of empty images: only the frame is drawn)
            hipLaunchKernelGGL(simplify_kernel, dim3((unsigned)A.nlines), dim3(64), 0, h->stream, A);
        VPK_HIP(h, t.mark(ChunkTimes::SIMPLIFY));
        hipLaunchKernelGGL(outline_kernel, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, h->stream, A);
        VPK_HIP(h, t.mark(ChunkTimes::OUTLINE));
        const int wgs = (int)std::min<long long>(nt, 3ll * h->num_cu);      // three workgroups fit a CU (LDS, registers)
        hipLaunchKernelGGL(coverage_kernel, dim3(wgs), dim3(RT), cov_dyn, h->stream, A);
        VPK_HIP(h, t.mark(ChunkTimes::COVERAGE));
        hipLaunchKernelGGL(blend_kernel, dim3((size + BROWS - 1) / BROWS, A.batch), dim3(BROWS * BSEG), blend_lds(size, A.a8), h->stream, A);
        VPK_HIP(h, t.mark(ChunkTimes::BLEND));
        VPK_HIP(h, hipGetLastError());
        VPK_HIP(h, t.report(A));
    }
    return VPK_OK;
}

/* per-image flags of the last vpk_sphere_raster call on this handle (bit 0: a line's outline or coverage exceeded the
 * kernel's buffers and was truncated / dropped); waits for the call to finish */
int vpk_sphere_raster_flags(vpk_handle* h, int batch, uint32_t* flags_out) {
    if (!h || !flags_out || batch < 1 || !h->raster_hdr) return vpk_fail(h, VPK_ERR_ARG, "vpk_sphere_raster_flags: bad argument");
    if (batch != h->raster_last_batch)                    // the flags' place in the workspace depends on the call's batch
        return vpk_fail(h, VPK_ERR_ARG, "vpk_sphere_raster_flags: batch differs from the last vpk_sphere_raster call's");
    VPK_HIP(h, hipSetDevice(h->device));
    VPK_HIP(h, hipStreamSynchronize(h->stream));
    const size_t flags = raster_layout(batch, 0, 0, 0, false).flags;      // (the layout's head depends on the batch alone)
    VPK_HIP(h, hipMemcpy(flags_out, (char*)h->raster_hdr + flags, (size_t)batch * 4, hipMemcpyDeviceToHost));
    return VPK_OK;
}

int vpk_sphere_raster_set_alternative(vpk_handle* h, int on) {
    if (!h) return VPK_ERR_ARG;
    if (h->raster_alternative != (on ? 1 : 0)) h->raster_offsets.clear();   // (the chunking, hence the cached image order, differs)
    h->raster_alternative = on ? 1 : 0;
    return VPK_OK;
}

}  // extern "C"
