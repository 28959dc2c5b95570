// sim_raster.cpp -- TEST-ONLY host build of the rasteriser (csrc/raster_device.hpp, raster_curve.hpp, raster_coverage.hpp,
// unmodified; see hip_sim.hpp): the curve's samples, the simplifier, the stroker, the split column, polygon_coverage -- row
// split, joined rows, bands, sweep, row table -- and the blender are the product's code, run by ONE thread on host arrays
// where the GPU has a workgroup on LDS.  Only what is around them is a serial loop here: line after line, each sub-path's
// polygon through polygon_coverage into the line's rows of the dense table, then the table's ranges blended in line and
// sub-path order.  (simplify_kernel's wave machine and blend_kernel's fetch pipeline and tables need a real 64-lane wave: GPU
// tests.)  It is not a product path: nothing in the package builds, loads or links it.
#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/raster_coverage.hpp"
#include "../../vanishing_points_2017_amd/csrc/raster_curve.hpp"

#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace vpk_raster;

namespace {

// what coverage_kernel keeps in LDS and in the call's workspace, for one line at a time
struct Canvas {
    int size, pool;
    std::vector<int> rows, pcover, parea;                 // six row arrays; the cell pool
    std::vector<unsigned char> alpha;                     // the line's alpha bytes (a canvas per sub-path: more than any line takes)
    std::vector<RowEnt> dense;                            // [MAXSUB][size]
    unsigned long long bump = 0;
    CovShared S;
    CellSink sink;
    CovOut O;
    long long split_rows = 0, joined_rows = 0, banded = 0;
    Canvas(int size_, int pool_) : size(size_), pool(pool_), rows(6 * (size_t)size_), pcover(pool_, 0), parea(pool_, 0),
                                   alpha((size_t)MAXSUB * size_ * (size_ + 2)), dense((size_t)MAXSUB * size_) {
        int* r = rows.data();
        sink.rowmin = r; sink.rowmax = r + size; sink.rowoff = r + 2 * size; sink.rmin = r + 3 * size; sink.rmax = r + 4 * size;
        sink.lcov = r + 5 * size;
        for (int y = 0; y < size; ++y) {                  // (as coverage_kernel starts; polygon_coverage leaves them so)
            sink.rowmin[y] = 0x7fffffff; sink.rowmax[y] = -1; sink.rowoff[y] = 0; sink.rmin[y] = 0x7fffffff; sink.rmax[y] = -1;
            sink.lcov[y] = 0;
        }
        sink.pcover = pcover.data(); sink.parea = parea.data();
        sink.size = size; sink.xs = 0; sink.blo = 0; sink.bhi = 0; sink.boff = 0;
        O.alpha = alpha.data(); O.alpha_cap = alpha.size(); O.bump = &bump; O.pool = pool; O.probe = 0; O.laps = nullptr;
    }
    // sub-path q (of npoly) of the line at hand -> its rows of the dense table; false: dropped
    bool cover(const V2* v, int n, int xsplit, int q, int npoly) {
        const int more = q == 0 ? (npoly > 1 ? npoly - 1 : 0) << ROW_MORE_SHIFT : 0;
        const unsigned long long before = bump;
        RowEnt* ent = dense.data() + (size_t)q * size;
        const bool ok = polygon_coverage(v, n, xsplit, sink, size, S, O, ent, more);
        banded += bump - before > (unsigned long long)pool;               // more entries than the pool holds: several bands
        for (int y = 0; y < size; ++y) {
            const Range l = range_l(ent[y]), r = range_r(ent[y]);
            split_rows += l.len > 0 && r.len > 0;
            joined_rows += l.len > 0 && r.len == 0 && l.xmin + l.len > xsplit;      // one range with cells on both sides
        }
        return ok;
    }
    void blend_range(const Range& r, int y, unsigned grey, unsigned a8, unsigned char* img) const {
        for (int q = 0; q < r.len; ++q) {
            const int x = r.xmin + q;
            const unsigned al = alpha[(size_t)r.off + q];
            if (al && x >= 0 && x < size) img[(size_t)y * size + x] = (unsigned char)blend(img[(size_t)y * size + x], grey, a8, al);
        }
    }
    // the line's rows as blend_kernel reads them: sub-path 0, then as many more as its `more` bits say
    void blend_line(unsigned grey, unsigned a8, unsigned char* img) {
        for (int y = 0; y < size; ++y) {
            const int more = (dense[y].lenL >> ROW_MORE_SHIFT) & 7;
            for (int q = 0; q <= more; ++q) {
                const RowEnt& e = dense[(size_t)q * size + y];
                blend_range(range_l(e), y, grey, a8, img);
                blend_range(range_r(e), y, grey, a8, img);
            }
        }
        bump = 0;
    }
};

// the samples of one line through the simplifier, as outline_kernel's sequential machine feeds them: `sub(n)` is called at the
// end of every sub-path that kept n >= 2 points (in simp[0 .. n)); returns the simplifier's overflow flag
template <class F>
unsigned line_subpaths(const double* l, int size, int alt, std::vector<V2>& simp, F sub) {
    const int ns = SAMPLES;
    Simplifier sm;
    sm.init(simp.data(), MAXS);
    auto flush = [&]() {
        sm.end();
        if (sm.n >= 2) sub(sm.n);
        sm.n = 0;
    };
    constexpr int OG = SAMPLE_GROUP;
    for (int i0 = 0; i0 < ns; i0 += OG) {
        double xs[OG], ys[OG];
        for (int u = 0; u < OG; ++u) {
            double s[3];
            curve_sample(i0 + u < ns ? i0 + u : ns - 1, ns, size, s);
            xs[u] = s[0];
            ys[u] = curve_y(curve_beta(l[0], l[1], l[2], s[1], s[2], alt), size);
        }
        feed_group<OG>(sm, xs, ys, ns - i0, flush);
    }
    if (sm.have) flush();
    return sm.overflow;
}

}  // namespace

// the pool size the product gives coverage_kernel for a canvas size
extern "C" int sim_raster_pool(int size) { return coverage_pool(size); }

// counters[0 .. 3), summed over the call: rows that kept two separate ranges, rows whose ranges were joined, polygons that
// took more than one band of the pool.  Returns the overflow flags, or -1 for a pool too small to hold one joined row (the band
// packing would overrun it).
extern "C" int sim_raster(const double* l, int nlines, int size, double alpha, int alt, int pool, unsigned char* out,
                          long long* counters) {
    if (pool < size + 2) return -1;
    std::vector<V2> simp(MAXS), verts(MAXV);
    Canvas cv(size, pool);
    memset(out, 0, (size_t)size * size);
    unsigned flags = 0;
    const unsigned a8 = (unsigned)(alpha * 255.0 + 0.5);
    for (int g = 0; g < nlines; ++g) {
        // outline_kernel: the line's polygons side by side in verts, up to MAXSUB of them
        Outline o;
        o.v = verts.data(); o.n = 0; o.cap = MAXV; o.flags = &flags;
        int npoly = 0, first[MAXSUB], count[MAXSUB], xsplit[MAXSUB];
        flags |= line_subpaths(l + 3 * g, size, alt, simp, [&](int n) {
            const int at = o.n, xs = split_column(simp.data(), n, size);
            stroke_outline(simp.data(), n, LINE_WIDTH_PX, o);
            if (o.n - at < 3) return;
            if (npoly < MAXSUB) { first[npoly] = at; count[npoly] = o.n - at; xsplit[npoly] = xs; ++npoly; }
            else flags |= FLAG_OVERFLOW;
        });
        if (npoly == 0) continue;
        for (int q = 0; q < npoly; ++q)
            if (!cv.cover(verts.data() + first[q], count[q], xsplit[q], q, npoly)) flags |= FLAG_OVERFLOW;
        cv.blend_line(255u, a8, out);
    }
    for (int side = 0; side < 4; ++side) {
        spine_path(side, size, simp.data());
        Outline o;
        o.v = verts.data(); o.n = 0; o.cap = MAXV; o.flags = &flags;
        stroke_outline(simp.data(), 2, SPINE_WIDTH_PX, o);
        if (!cv.cover(verts.data(), o.n, size + 2, 0, 1)) flags |= FLAG_OVERFLOW;      // (a spine: one range per row)
        cv.blend_line(0u, 255u, out);
    }
    counters[0] = cv.split_rows; counters[1] = cv.joined_rows; counters[2] = cv.banded;
    return (int)flags;
}

// the cells of ONE edge walked whole (nparts = 1) and in shares (nparts = K): the closed-form restart of AGG's row DDA must give
// the same accumulators.  Returns the number of accumulator entries that differ.  The accumulators are image-sized, [size][size
// + 2] with x shifted by one (cells at x = -1 and x = size exist), behind identity row tables.
extern "C" int sim_edge_shares(double x1, double y1, double x2, double y2, int size, int K) {
    std::vector<int> c1((size_t)size * (size + 2), 0), a1(c1), c2(c1), a2(c1), rowoff(size), rowmin(size, 0), lcov(size, -1);
    for (int y = 0; y < size; ++y) rowoff[y] = y * (size + 2);
    CellSink s;
    s.rowmin = rowmin.data(); s.rowmax = nullptr; s.rowoff = rowoff.data(); s.size = size;
    s.rmin = s.rmax = nullptr; s.lcov = lcov.data(); s.xs = 0x7fffffff;
    s.blo = 0; s.bhi = size; s.boff = 0;
    EdgeClip ec;
    ec.bx1 = 0.0; ec.by1 = 0.0; ec.bx2 = (double)size; ec.by2 = (double)size;
    s.pcover = c1.data(); s.parea = a1.data();
    ec.c = s;
    ec.nparts = 1; ec.part = 0;
    ec.edge<POOLED>(x1, y1, x2, y2);
    s.pcover = c2.data(); s.parea = a2.data();
    ec.c = s;
    ec.nparts = K;
    for (int q = 0; q < K; ++q) { ec.part = q; ec.edge<POOLED>(x1, y1, x2, y2); }
    int bad = 0;
    for (size_t i = 0; i < c1.size(); ++i) bad += (c1[i] != c2[i]) || (a1[i] != a2[i]);
    return bad;
}

// the outline polygons the product's simplifier and stroker make of ONE line: the vertex count of every sub-path that is
// drawn (>= 3 vertices), in path order, into counts[0 .. max); returns how many there are (the kernels keep up to MAXSUB and
// hold a polygon's vertices in LDS up to a limit: the tests look for lines on both sides of it)
extern "C" int sim_outline_counts(const double* l, int size, int alt, int* counts, int max) {
    std::vector<V2> simp(MAXS), verts(MAXV);
    unsigned flags = 0;
    int np = 0;
    line_subpaths(l, size, alt, simp, [&](int n) {
        Outline o;
        o.v = verts.data(); o.n = 0; o.cap = MAXV; o.flags = &flags;
        stroke_outline(simp.data(), n, LINE_WIDTH_PX, o);
        if (o.n >= 3) { if (np < max) counts[np] = o.n; ++np; }
    });
    return np;
}
