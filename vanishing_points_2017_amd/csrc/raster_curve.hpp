// raster_curve.hpp -- what the reference's plot call fixes before any path reaches Agg (sphere_mapping.py:36-72): the samples of
// alpha, the curve beta(alpha) and its place on the canvas, the axes' spines, the stroke widths -- and the column at which the
// coverage stage splits a curve's rows.  Called by the kernels of vpk_raster.hip and, unmodified, by the test-only host build
// tests/hostsim/sim_raster.cpp; both are built with -ffp-contract=off: every operation rounds as NumPy's separate ufunc calls.
#ifndef VPK_RASTER_CURVE_HPP_
#define VPK_RASTER_CURVE_HPP_

#include "raster_device.hpp"

namespace vpk_raster {

constexpr int SAMPLES = 10000;                           // sphere_mapping.py:40
constexpr int SAMPLE_GROUP = 4;                          // samples the sequential machine evaluates side by side (feed_group)
constexpr double LINE_WIDTH_PX = 100.0 / 72.0;           // 1 pt at 100 dpi (matplotlib 1.5.1's default line width)
constexpr double SPINE_WIDTH_PX = 0.8 * 100.0 / 72.0;    // the axes' spines: 0.8 pt

// sample i of ns, the same for every line, into xsc[0 .. 3): the pixel x of alpha (the axes' transform: always finite), sin and
// cos of alpha (sphere_mapping.py:61-63)
RDEV_INLINE void curve_sample(int i, int ns, int size, double* xsc) {
    const double lo_a = -PI_D / 2, hi_a = PI_D / 2;
    const double step = (hi_a - lo_a) / (ns - 1);
    const double al = (i == ns - 1) ? hi_a : lo_a + i * step;       // numpy.linspace
    xsc[0] = (al - lo_a) / (hi_a - lo_a) * size;
    xsc[1] = sin(al);
    xsc[2] = cos(al);
}

// beta(alpha) of one sample, operation by operation as NumPy evaluates the reference's expression (sphere_mapping.py:59 /
// :61, then `b *= -1`, :63)
RDEV_INLINE double curve_beta(double la, double lb, double lc, double sa, double ca, int alt) {
    double be = alt ? -atan(-lc / (ca * la + sa * lb))                     // :59
                    : -atan((-la * sa - lc * ca) / lb);                   // :61
    be *= -1;                                                             // :63
    return be;
}
// the axes' transform of beta: the pixel y of a sample
RDEV_INLINE double curve_y(double be, int size) {
    const double lo_a = -PI_D / 2, hi_a = PI_D / 2;
    return size - (be - lo_a) / (hi_a - lo_a) * size;
}

// the axes' spines: left, right, bottom, top (matplotlib's drawing order): two-vertex rectilinear paths, snapped to pixel
// centres (PathSnapper: floor(v + 0.5) + 0.5 for a stroke whose width rounds to an odd number of pixels)
RDEV_INLINE void spine_path(int side, int size, V2* sp) {
    const double s = (double)size;
    const double x0 = (side == 1) ? s : 0.0, y0 = (side == 3) ? 0.0 : s;
    const double x1 = (side == 0) ? 0.0 : s, y1 = (side == 2) ? s : 0.0;
    sp[0].x = floor(x0 + 0.5) + 0.5; sp[0].y = floor(y0 + 0.5) + 0.5;
    sp[1].x = floor(x1 + 0.5) + 0.5; sp[1].y = floor(y1 + 0.5) + 0.5;
}

// the column at which the coverage stage splits the rows' cells in two ranges (raster_device.hpp: CellSink): the curve's
// interior extremum (a row beside it is crossed twice, far apart); any column is correct, this one saves the most.  From the
// kept points of the path.
RDEV_INLINE int split_column(const V2* p, int n, int size) {
    int imin = 0, imax = 0;
    for (int k = 1; k < n; ++k) { if (p[k].y < p[imin].y) imin = k; if (p[k].y > p[imax].y) imax = k; }
    const double xa = p[imin].x, xb = p[imax].x;
    const double da = xa < size - xa ? xa : size - xa, db = xb < size - xb ? xb : size - xb;   // distance from the canvas's sides
    const double x = da >= db ? xa : xb;
    const int c = (int)floor(x);
    return c < 0 ? 0 : (c > size ? size : c);
}

}  // namespace vpk_raster
#endif
