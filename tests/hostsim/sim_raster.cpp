// sim_raster.cpp -- TEST-ONLY host build of the rasteriser's arithmetic (csrc/raster_device.hpp, unmodified): the
// simplifier, the stroker, the cell walker with its clip box, calculate_alpha and the blender are the product's code; only
// the orchestration around them -- which on the GPU is three kernels, LDS pools and atomics -- is a serial loop here
// (samples -> outline per line; cells of one polygon into image-sized accumulators; sweep per row; blend; next line).
// It is not a product path: nothing in the package builds, loads or links it.
#include "../../vanishing_points_2017_amd/csrc/raster_device.hpp"

#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace vpk_raster;

namespace {

void draw_polygon(const V2* v, int n, unsigned grey, unsigned a8, int size, std::vector<int>& cover, std::vector<int>& area,
                  std::vector<int>& rowmin, std::vector<int>& rowmax, unsigned char* img) {
    CellSink sink;
    sink.cover = cover.data(); sink.area = area.data(); sink.pcover = nullptr; sink.parea = nullptr;
    sink.rowmin = rowmin.data(); sink.rowmax = rowmax.data(); sink.rowoff = nullptr; sink.size = size;
    sink.rmin = sink.rmax = sink.lcov = nullptr; sink.xs = 0x7fffffff;      // one range per row here
    sink.blo = 0; sink.bhi = size; sink.boff = 0;
    EdgeClip ec;
    ec.bx1 = 0.0; ec.by1 = 0.0; ec.bx2 = (double)size; ec.by2 = (double)size; ec.c = sink;
    ec.nparts = 1; ec.part = 0;          // the cells: every edge whole, into image-sized accumulators
    for (int k = 0; k < n; ++k) ec.edge<GLOBAL>(v[k].x, v[k].y, v[k + 1 < n ? k + 1 : 0].x, v[k + 1 < n ? k + 1 : 0].y);
    ec.nparts = 16;                      // the bounds pass the way the GPU runs it: every share of every edge
    for (int k = 0; k < n; ++k)
        for (int q = 0; q < 16; ++q) {
            ec.part = q;
            ec.edge<BOUNDS>(v[k].x, v[k].y, v[k + 1 < n ? k + 1 : 0].x, v[k + 1 < n ? k + 1 : 0].y);
        }
    const int ldc = size + 2;
    for (int y = 0; y < size; ++y) {
        const int lo = rowmin[y], hi = rowmax[y];
        if (hi < lo) continue;
        int R = 0;
        for (int xi = lo; xi <= hi; ++xi) {               // the per-pixel form of sweep_scanline (coverage_kernel)
            int& c = cover[(size_t)y * ldc + xi];
            int& a = area[(size_t)y * ldc + xi];
            R += c;
            unsigned al = 0;
            if (a) al = calc_alpha((R << (SHIFT + 1)) - a);
            else if (xi < hi) al = calc_alpha(R << (SHIFT + 1));
            c = 0; a = 0;
            const int x = xi - 1;
            if (al && x >= 0 && x < size) img[(size_t)y * size + x] = (unsigned char)blend(img[(size_t)y * size + x], grey, a8, al);
        }
        rowmin[y] = 0x7fffffff;
        rowmax[y] = -1;
    }
}

// the samples of one line through the simplifier, as outline_kernel's sequential machine feeds them: `sub(n)` is called at the
// end of every sub-path that kept n >= 2 points (in simp[0 .. n)); returns the simplifier's overflow flag
template <class F>
unsigned line_subpaths(const double* l, int size, int alt, std::vector<V2>& simp, F sub) {
    const int ns = 10000;
    const double lo_a = -PI_D / 2, hi_a = PI_D / 2, step = (hi_a - lo_a) / (ns - 1);
    const double la = l[0], lb = l[1], lc = l[2];
    Simplifier sm;
    sm.init(simp.data(), MAXS);
    auto flush = [&]() {
        sm.end();
        if (sm.n >= 2) sub(sm.n);
        sm.n = 0;
    };
    constexpr int OG = 8;                                     // groups, as outline_kernel feeds them
    for (int i0 = 0; i0 < ns; i0 += OG) {
        double xs[OG], ys[OG];
        for (int u = 0; u < OG; ++u) {
            const int i = i0 + u < ns ? i0 + u : ns - 1;
            const double al = (i == ns - 1) ? hi_a : lo_a + i * step;
            double be = alt ? -atan(-lc / (cos(al) * la + sin(al) * lb))      // sphere_mapping.py:59
                            : -atan((-la * sin(al) - lc * cos(al)) / lb);     // :61
            be *= -1;
            xs[u] = (al - lo_a) / (hi_a - lo_a) * size;
            ys[u] = size - (be - lo_a) / (hi_a - lo_a) * size;
        }
        feed_group<OG>(sm, xs, ys, ns - i0, flush);
    }
    if (sm.have) flush();
    return sm.overflow;
}

}  // namespace

extern "C" int sim_raster(const double* l, int nlines, int size, double alpha, int alt, unsigned char* out) {
    std::vector<V2> simp(MAXS), verts(MAXV);
    std::vector<int> cover((size_t)size * (size + 2), 0), area((size_t)size * (size + 2), 0), rowmin(size, 0x7fffffff), rowmax(size, -1);
    memset(out, 0, (size_t)size * size);
    unsigned flags = 0;
    const unsigned a8 = (unsigned)(alpha * 255.0 + 0.5);
    for (int g = 0; g < nlines; ++g) {
        const unsigned overflow = line_subpaths(l + 3 * g, size, alt, simp, [&](int n) {
            Outline o;
            o.v = verts.data(); o.n = 0; o.cap = MAXV; o.flags = &flags;
            stroke_outline(simp.data(), n, 100.0 / 72.0, o);
            if (o.n >= 3) draw_polygon(verts.data(), o.n, 255u, a8, size, cover, area, rowmin, rowmax, out);
        });
        flags |= overflow;
    }
    const double s = (double)size, w_spine = 0.8 * 100.0 / 72.0;
    for (int side = 0; side < 4; ++side) {
        const double x0 = (side == 1) ? s : 0.0, y0 = (side == 3) ? 0.0 : s, x1 = (side == 0) ? 0.0 : s, y1 = (side == 2) ? s : 0.0;
        simp[0].x = floor(x0 + 0.5) + 0.5; simp[0].y = floor(y0 + 0.5) + 0.5;
        simp[1].x = floor(x1 + 0.5) + 0.5; simp[1].y = floor(y1 + 0.5) + 0.5;
        Outline o;
        o.v = verts.data(); o.n = 0; o.cap = MAXV; o.flags = &flags;
        stroke_outline(simp.data(), 2, w_spine, o);
        draw_polygon(verts.data(), o.n, 0u, 255u, size, cover, area, rowmin, rowmax, out);
    }
    return (int)flags;
}

// the cells of ONE edge walked whole (nparts = 1) and in shares (nparts = K): the closed-form restart of AGG's row DDA must give
// the same accumulators.  Returns the number of accumulator entries that differ.
extern "C" int sim_edge_shares(double x1, double y1, double x2, double y2, int size, int K) {
    std::vector<int> c1((size_t)size * (size + 2), 0), a1(c1), c2(c1), a2(c1), rmin(size, 0x7fffffff), rmax(size, -1);
    CellSink s;
    s.pcover = s.parea = nullptr; s.rowmin = rmin.data(); s.rowmax = rmax.data(); s.rowoff = nullptr; s.size = size;
    s.rmin = s.rmax = s.lcov = nullptr; s.xs = 0x7fffffff;
    s.blo = 0; s.bhi = size; s.boff = 0;
    EdgeClip ec;
    ec.bx1 = 0.0; ec.by1 = 0.0; ec.bx2 = (double)size; ec.by2 = (double)size;
    s.cover = c1.data(); s.area = a1.data();
    ec.c = s;
    ec.nparts = 1; ec.part = 0;
    ec.edge<GLOBAL>(x1, y1, x2, y2);
    s.cover = c2.data(); s.area = a2.data();
    ec.c = s;
    ec.nparts = K;
    for (int q = 0; q < K; ++q) { ec.part = q; ec.edge<GLOBAL>(x1, y1, x2, y2); }
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
        stroke_outline(simp.data(), n, 100.0 / 72.0, o);
        if (o.n >= 3) { if (np < max) counts[np] = o.n; ++np; }
    });
    return np;
}
