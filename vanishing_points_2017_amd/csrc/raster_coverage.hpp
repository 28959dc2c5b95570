// raster_coverage.hpp -- the coverage stage of the sphere rasteriser: one outline polygon -> its alpha bytes and its rows in
// the dense row table.  coverage_kernel (vpk_raster.hip) calls polygon_coverage with a workgroup of RT threads on LDS arrays;
// the test-only host build tests/hostsim/sim_raster.cpp compiles this file unmodified and calls it with ONE thread on host
// arrays (RT = 1, WAVE = 1: tests/hostsim/hip_sim.hpp), so that the CPU suite runs the row split, the joined rows, the bands
// and the row table themselves.  Written against the vocabulary of wave_prims.hpp and raster_device.hpp only.
#ifndef VPK_RASTER_COVERAGE_HPP_
#define VPK_RASTER_COVERAGE_HPP_

#include "wave_prims.hpp"
#include "raster_device.hpp"

namespace vpk_raster {

// One polygon's coverage of one image row: up to two ranges of pixels (raster_device.hpp: CellSink) whose alpha bytes lie back
// to back in the call's pool -- L: pixels [xminL, xminL + lenL) at `off`, R: [xminR, xminR + lenR) at off + lenL (a length
// of 0: no such range; both 0: the row is not touched).  The table is DENSE -- [line][sub-path][row] -- so that the blend can
// fetch the entries of several lines at once without first reading anything about the lines; bits 12.. of `lenL` in
// sub-path 0 = the line's further sub-paths (a NaN sample breaks the path: rare).
struct RowEnt { unsigned off; short xminL, lenL, xminR, lenR; int pad; };
constexpr int ROW_LEN = 0xfff, ROW_MORE_SHIFT = 12;

struct Range { unsigned off; int xmin, len; };            // one range of an entry: pixels [xmin, xmin + len), bytes at off
RDEV_INLINE Range range_l(const RowEnt& e) { Range r; r.off = e.off; r.xmin = e.xminL; r.len = e.lenL & ROW_LEN; return r; }
RDEV_INLINE Range range_r(const RowEnt& e) {
    Range r; r.off = e.off + (unsigned)(e.lenL & ROW_LEN); r.xmin = e.xminR; r.len = e.lenR; return r;
}
RDEV_INLINE RowEnt untouched_row(int more) {              // a row the polygon leaves alone (more: the "further sub-paths" bits)
    RowEnt r;
    r.off = 0; r.xminL = 0; r.lenL = (short)more; r.xminR = 0; r.lenR = 0; r.pad = 0;
    return r;
}

// coverage_kernel's LDS: three workgroups per CU (53 KB each); what the static arrays (CovShared and the kernel's queue word,
// at most COV_STATIC bytes) and the six row arrays leave is the pool.  (Measured with the two-range rows, 102 / 95 images:
// 512 threads x 2 per CU 1.36 / 2.60 ms, 256 x 4 1.32 / 2.23, 256 x 3 1.06 / 1.98.)
constexpr int COV_LDS = 53 * 1024, COV_STATIC = 11 * 1024;
constexpr int MAX_SIZE = 1024;                           // the largest canvas (ROW_LEN and the LDS budgets are sized for it)
constexpr int coverage_rowcap(int size) { return (size + 63) & ~63; }
// pool entries (cover, area) for a canvas size: at least size + 2, one joined row, must fit
constexpr int coverage_pool(int size) { return ((COV_LDS - COV_STATIC - 6 * coverage_rowcap(size) * 4) / 8) & ~63; }
static_assert(coverage_pool(MAX_SIZE) >= MAX_SIZE + 2, "a band of the pool must hold one joined row");

constexpr int LVERT = 256;                               // vertices of a polygon held in LDS (typical: 60-200)
struct CovShared {                                       // ALL of coverage_kernel's static LDS: scratch for the polygon at hand
    V2 vert[LVERT + 1];                                  // its vertices (closed: [n] = [0])
    unsigned short eoff[MAXV + 2];                       // first work item of every edge
    int next;                                            // (the kernel's own: the next line of its queue)
    int ymax, ymin;                                      // last / first touched row
    int tail[2 * RT];                                    // the sweep's per-thread partial sums
    long long base[2];                                   // [0]: the polygon's place in the call's alpha pool, -1: dropped
    int total;                                           // entries of all its rows
};                                                       // (the order: the offsets the kernel was measured with)
static_assert(sizeof(CovShared) <= COV_STATIC, "coverage_kernel's static LDS exceeds what coverage_pool() leaves for it");
// where the polygons' alpha bytes go (the call's pool in HBM, space by one 64-bit bump counter), how large the cell pool
// behind CellSink::pcover / parea is, and the development probe (workgroup 0 adds its phases' clock ticks to laps[0..3])
struct CovOut {
    unsigned char* alpha; unsigned long long alpha_cap; unsigned long long* bump;
    int pool;
    int probe; int* laps;
};

// cells of one polygon -> coverage bytes: bounds pass, row scan, cells into the LDS pool, sweep -> alpha bytes in the pool's
// packing.  A workgroup spends most of a polygon waiting -- on barriers and on memory round trips -- so the round trips
// are kept off the critical path: the vertices are fetched once (LDS), a thread keeps its work item between the two
// passes, the pools' space comes from ONE atomic, the next line's number is requested a polygon ahead.
// Returns false if the polygon was dropped (the call's HBM pool is full): its rows are then written as untouched.
RDEV bool polygon_coverage(const V2* v, int n, int xsplit, const CellSink& sink, int size, CovShared& S, const CovOut& A,
                           RowEnt* ent, int more) {
    const int t = vpk::tid();
    const bool probe = A.probe && t == 0 && vpk::block_id() == 0;
    long long tp = probe ? vpk::clock_ticks() : 0;
    auto lap = [&](int slot) {
        if (probe) { const long long now = vpk::clock_ticks(); vpk::atomic_add_int(A.laps + slot, (int)(now - tp)); tp = now; }
    };
    unsigned short* s_eoff = S.eoff;
    const int POOL = A.pool;
    EdgeClip ec;
    ec.bx1 = 0.0; ec.by1 = 0.0; ec.bx2 = (double)size; ec.by2 = (double)size; ec.c = sink;
    ec.c.xs = xsplit;
    // Work items = (edge, share of its rows).  An outline has ~120 edges of which most cross one to three rows and a few
    // thirty or more; an item costs the clipper's and the walker's set-up (divisions in double and in int) before its first
    // cell, so an edge gets one share per ROWS_PER_ITEM rows it crosses -- not a fixed number of shares (with 4 RT / n
    // shares per edge, 9 in 10 items were empty and the set-up was most of the kernel).  The shares' offsets: one wave's scan.
    constexpr int ROWS_PER_ITEM = 4;
    const bool inlds = n <= LVERT;
    for (int k = t; k < n; k += RT) {
        const V2 a = v[k];
        const double ya = a.y, yb = v[k + 1 < n ? k + 1 : 0].y;
        if (inlds) { S.vert[k] = a; if (k == 0) S.vert[n] = a; }
        double lo = ya < yb ? ya : yb, hi = ya < yb ? yb : ya;
        lo = lo > 0.0 ? lo : 0.0;
        hi = hi < (double)size ? hi : (double)size;
        const int rows = hi >= lo ? (int)hi - (int)lo + 1 : 1;      // (an estimate is enough: any split gives the same cells)
        int ke = (rows + ROWS_PER_ITEM - 1) / ROWS_PER_ITEM;
        s_eoff[k] = (unsigned short)(ke > 32 ? 32 : ke);
    }
    vpk::block_sync();
    // (both prefix sums below: the first wave's lane t takes `per` consecutive items, one wave_scan_int over the lanes' sums.
    //  The loops around it are written out twice: behind a common helper that takes the item's length as a function, the
    //  compiler allocates and schedules the whole kernel differently -- 125 instead of 132 VGPRs -- which wants measuring)
    if (t < vpk::WAVE) {
        const int per = (n + vpk::WAVE - 1) / vpk::WAVE, k0 = t * per;
        int sum = 0;
        for (int k = k0; k < k0 + per && k < n; ++k) sum += s_eoff[k];
        const int incl = vpk::wave_scan_int(sum);
        int off = incl - sum;
        for (int k = k0; k < k0 + per && k < n; ++k) { const int ke = s_eoff[k]; s_eoff[k] = (unsigned short)off; off += ke; }
        if (t == vpk::WAVE - 1) s_eoff[n] = (unsigned short)incl;
    }
    vpk::block_sync();
    const int items = s_eoff[n];
    struct Work { int part, nparts; V2 a, b; };
    auto work_item = [&](int it) {                        // the edge whose shares contain item `it`: last k with eoff[k] <= it
        int lo = 0, hi = n;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int)s_eoff[mid] <= it) lo = mid; else hi = mid; }
        Work w;
        w.part = it - s_eoff[lo];
        w.nparts = s_eoff[lo + 1] - s_eoff[lo];
        if (inlds) { w.a = S.vert[lo]; w.b = S.vert[lo + 1]; }
        else { w.a = v[lo]; w.b = v[lo + 1 < n ? lo + 1 : 0]; }
        return w;
    };
    Work mine = {};                                       // this thread's first item: the same in both passes
    if (t < items) mine = work_item(t);
    for (int it = t; it < items; it += RT) {              // pass 1: the rows' cell ranges (L and R of the split column)
        const Work w = it == t ? mine : work_item(it);
        ec.part = w.part; ec.nparts = w.nparts;
        ec.edge<BOUNDS>(w.a.x, w.a.y, w.b.x, w.b.y);
    }
    vpk::block_sync();
    lap(0);
    // A row's pool entries: its L range then its R range, or -- if they touch, or if something is to be drawn between them
    // (lcov != 0) -- ONE range from the first L cell to the last R cell.  lcov becomes the number of L entries (-1: joined).
    auto row_entries = [&](int y) {
        const int sp = sink.lcov[y];
        return sp < 0 ? sink.rmax[y] - sink.rowmin[y] + 1 : sp + row_len(sink.rmin[y], sink.rmax[y]);
    };
    // exclusive prefix sum of the rows' entries (one wave), first / last touched row
    if (t < vpk::WAVE) {
        const int per = (size + vpk::WAVE - 1) / vpk::WAVE, y0 = t * per;
        int sum = 0, ymin = 0x7fffffff, ymax = -1;
        for (int y = y0; y < y0 + per && y < size; ++y) {
            const int ll = row_len(sink.rowmin[y], sink.rowmax[y]), rl = row_len(sink.rmin[y], sink.rmax[y]);
            const bool joined = ll > 0 && rl > 0 && (sink.rowmax[y] + 1 >= sink.rmin[y] || sink.lcov[y] != 0);
            sink.lcov[y] = joined ? -1 : ll;
            const int len = joined ? sink.rmax[y] - sink.rowmin[y] + 1 : ll + rl;
            if (len) { ymin = ymin < y ? ymin : y; ymax = y; }
            sum += len;
        }
        const int incl = vpk::wave_scan_int(sum);
        int off = incl - sum;
        for (int y = y0; y < y0 + per && y < size; ++y) { sink.rowoff[y] = off; off += row_entries(y); }
        ymin = vpk::wave_min_int(ymin);
        ymax = vpk::wave_max_int(ymax);
        if (t == vpk::WAVE - 1) {
            S.total = incl; S.ymin = ymin; S.ymax = ymax;
            long long ab = -1;
            if (incl > 0) {
                // space in the call's coverage pool: one atomic add; a polygon that does not fit gives its bytes back, so that
                // it alone is dropped (and its image flagged), not every polygon that asks after it.  (A compare-and-swap loop
                // on the one counter, 512 workgroups contending, cost 100 ms per call.)
                const unsigned long long old = vpk::atomic_add_u64(A.bump, (unsigned long long)incl);
                if (old + (unsigned long long)incl > A.alpha_cap) vpk::atomic_add_u64(A.bump, 0ull - (unsigned long long)incl);
                else ab = (long long)old;
            }
            S.base[0] = ab;
        }
    }
    vpk::block_sync();
    lap(1);
    const int total = S.total, ymin = S.ymin, ymax = S.ymax;
    const long long ab = S.base[0];
    const bool ok = ab >= 0;                              // (a polygon past the call's HBM pool is dropped and flagged)
    // The LDS pool holds the entries of a BAND of rows at a time: all touched rows when they fit (the usual case), else as
    // many consecutive rows as fit.
    int ys = ok ? ymin : size;
    while (ys <= ymax && ys < size) {
        int ye = ys + 1;                                  // (uniform: every thread walks the same prefix sums)
        const int boff = sink.rowoff[ys];
        if (total <= POOL) ye = ymax + 1;                  // everything fits: one band
        else while (ye <= ymax && sink.rowoff[ye] + row_entries(ye) - boff <= POOL) ++ye;
        CellSink band = ec.c;
        band.blo = ys; band.bhi = ye; band.boff = boff;
        ec.c = band;
        for (int it = t; it < items; it += RT) {          // pass 2: the cells of the band's rows
            const Work w = it == t ? mine : work_item(it);
            ec.part = w.part; ec.nparts = w.nparts;
            ec.edge<POOLED>(w.a.x, w.a.y, w.b.x, w.b.y);
        }
        vpk::block_sync();
        lap(2);
        // The sweep (the per-pixel form of sweep_scanline, see blend_kernel) over the band's pool entries, which are the
        // rows' entries back to back: every thread takes an equal run of consecutive entries -- not a row: rows are 1
        // to 500 entries long --, the running cover at the start of its run being the covers of its row before it.  (The
        // running cover simply continues from a row's L entries into its R entries: it is 0 across a dropped gap.)
        const int last = ye - 1;
        const int bend = sink.rowoff[last] + row_entries(last);
        const int E = bend - boff, C = (E + RT - 1) / RT;
        const int q0 = t * C, q1 = q0 + C < E ? q0 + C : E;
        int y = ys, row_lo = 0, row_hi = 0;               // the row of entry q0: pool entries [row_lo, row_hi)
        auto row_span = [&](int yy) { row_lo = sink.rowoff[yy] - boff; row_hi = row_lo + row_entries(yy); };
        if (q0 < q1) {
            int lo = ys, hi = ye;                         // last row whose offset is <= q0 (an empty row shares its successor's)
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (sink.rowoff[mid] - boff <= q0) lo = mid; else hi = mid; }
            y = lo;
            row_span(y);
            int tail = 0, started = 0, yy = y, rhi = row_hi;
            for (int q = q0; q < q1; ++q) {
                if (q == rhi) {                           // the next non-empty row starts at this entry
                    do { ++yy; rhi = sink.rowoff[yy] - boff + row_entries(yy); } while (q == rhi);
                    tail = 0; started = 1;
                }
                tail += sink.pcover[q];
            }
            if (q0 == row_lo) started = 1;
            S.tail[2 * t] = tail; S.tail[2 * t + 1] = started;
        }
        vpk::block_sync();
        if (q0 < q1) {
            int R = 0;
            if (q0 != row_lo)
                for (int u = t - 1; u >= 0; --u) { R += S.tail[2 * u]; if (S.tail[2 * u + 1]) break; }
            for (int q = q0; q < q1; ++q) {
                if (q == row_hi) { do { ++y; row_span(y); } while (q == row_hi); R = 0; }
                const int c = sink.pcover[q], a = sink.parea[q];
                sink.parea[q] = 0;
                R += c;
                unsigned al = 0;
                if (a) al = calc_alpha((R << (SHIFT + 1)) - a);
                else if (q + 1 < row_hi) al = calc_alpha(R << (SHIFT + 1));
                sink.pcover[q] = (int)al;                 // the alphas stay in the pool ...
            }
        }
        for (int yy = ys + t; yy < ye; yy += RT) {
            const int sp = sink.lcov[yy];
            const int ll = sp < 0 ? sink.rmax[yy] - sink.rowmin[yy] + 1 : sp, rl = sp < 0 ? 0 : row_len(sink.rmin[yy], sink.rmax[yy]);
            RowEnt r;
            r.off = (unsigned)(ab + sink.rowoff[yy]);
            r.xminL = (short)(ll ? sink.rowmin[yy] - 1 : 0); r.lenL = (short)(ll | more);
            r.xminR = (short)(rl ? sink.rmin[yy] - 1 : 0); r.lenR = (short)rl;
            r.pad = 0;
            ent[yy] = r;
        }
        vpk::block_sync();
        {   // ... and leave it in one coalesced copy (the pool is zero again afterwards)
            unsigned char* dst = A.alpha + ab + boff;
            for (int q = t; q < E; q += RT) { dst[q] = (unsigned char)sink.pcover[q]; sink.pcover[q] = 0; }
        }
        vpk::block_sync();
        lap(3);
        ys = ye;
    }
    for (int y = t; y < size; y += RT) {
        if (!ok || y < ymin || y > ymax) ent[y] = untouched_row(more);      // rows the polygon leaves alone
        sink.rowmin[y] = 0x7fffffff; sink.rowmax[y] = -1; sink.rmin[y] = 0x7fffffff; sink.rmax[y] = -1; sink.lcov[y] = 0;
    }
    vpk::block_sync();
    return ok || total == 0;
}

}  // namespace vpk_raster
#endif
