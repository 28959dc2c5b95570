// lsd_device.hpp -- the line segment detector of the front end: the one source of its arithmetic, for the host
// (vpk_lsd_detect: lsd_host.hpp, vpk_lsd.cpp) and for the GPU batch (vpk_lsd_detect_batch: vpk_lsd_gpu.hip).
//
// replaces: lsdpython.lsd.detect_line_segments(image) as called from detect_lsd_lines (evaluation.py:227-251).
// The reference's detector lives in an un-vendored submodule (.gitmodules:1-3 -> github.com/fkluger/lsd-python, a
// Cython wrapper around R. Grompone von Gioi's LSD 1.6; the directory is empty in the reference), so there is no
// source to follow and no output to pin against: PARITY UNPINNED.  This file restates the PUBLISHED algorithm --
// Grompone von Gioi, Jakubowicz, Morel, Randall, "LSD: a Line Segment Detector", Image Processing On Line 2 (2012),
// with that paper's default parameters (scale 0.8, sigma_scale 0.6, quant 2.0, ang_th 22.5 deg, log_eps 0,
// density_th 0.7, n_bins 1024) -- step by step:
//   1. Gaussian sub-sampling to 80 %,                      2. gradient with a 2 x 2 mask, level-line angle, magnitude,
//   3. pixels pseudo-ordered by magnitude (1024 bins),     4. region growing with the region's running angle,
//   5. rectangle from the region's weighted inertia,       6. density check / refinement (angle tolerance, radius),
//   7. a-contrario validation: NFA = N_tests * binomial tail, kept if -log10(NFA) > 0, with the rectangle variations
//      of the paper's "rect_improve".
// Output rows: x1, y1, x2, y2, width, p, -log10(NFA) in pixel coordinates of the input image (7 doubles), the layout
// detect_lsd_lines consumes (columns 0..3 and 6).
//
// The steps are cut into per-pixel functions for the image-sized passes and one per-image driver (Region) for the
// sequential region stage.  hipcc compiles them into the kernels of vpk_lsd_gpu.hip and, with a one-lane wave, into
// vpk_lsd_detect; g++ compiles them, with LSD_HD empty, into the host build of the tests (tests/hostsim/sim_lsd.cpp).
// tests/golden/lsd/lsd_portable.npz holds rows recorded when the host detector was still written out on its own and equal
// to these functions bit for bit.
//
// What the GPU computes differently from the host is only the device libm (ocml): atan2 / sin / cos in the gradient and
// the region's running angle, exp / log / log10 / pow / sinh in the NFA.  Everything else -- the Gaussian weights (made
// on the host by gaussian_weights below), sqrt, division, floor / ceil, the integer pixel counts of the NFA, min / max --
// is exact and identical.  The elementary functions of the per-pixel and region-stage code go through a math policy M:
// Libm (the product's, above) or Portable (lsd_portable_math.hpp, test-only), under which device and host give the
// same bits and the kernels' orchestration is pinned exactly (tests/test_gpu_lsd_exact.py).  The fp64 sums of the region
// stage keep one order everywhere: on the GPU one wave runs the region stage of one image with every lane executing the
// same sequential code; only order-free work (the per-column pixel counts of rect_nfa and the min / max of region2rect)
// is split across the lanes.
#ifndef VPK_LSD_DEVICE_HPP_
#define VPK_LSD_DEVICE_HPP_

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "lsd_portable_math.hpp"

#ifdef __HIPCC__
#define LSD_HD __host__ __device__
#else
#define LSD_HD
#endif

namespace vpk_lsd {

constexpr double NOTDEF = -1024.0;
constexpr double PI_L = 3.14159265358979323846;
constexpr double M_3_2_PI_L = 4.71238898038;
constexpr double M_2__PI_L = 6.28318530718;
constexpr double LN10_L = 2.30258509299404568402;
constexpr int N_BINS = 1024;
// LSD's default parameters
constexpr double SIGMA_SCALE = 0.6, QUANT = 2.0, ANG_TH = 22.5, LOG_EPS = 0.0, DENSITY_TH = 0.7;

struct Pt { int x, y; };
struct Rect {
    double x1, y1, x2, y2, width, x, y, theta, dx, dy, prec, p;
};

// math policies of the device-side code (the host-only helpers below call glibc directly)
struct Libm {                                  // the product: ocml on the device, the C library on the host
    LSD_HD static double atan2(double y, double x) { return ::atan2(y, x); }
    LSD_HD static double sin(double x) { return ::sin(x); }
    LSD_HD static double cos(double x) { return ::cos(x); }
    LSD_HD static double exp(double x) { return ::exp(x); }
    LSD_HD static double log(double x) { return ::log(x); }
    LSD_HD static double log10(double x) { return ::log10(x); }
    LSD_HD static double pow(double x, double y) { return ::pow(x, y); }
    LSD_HD static double sinh(double x) { return ::sinh(x); }
};
struct Portable {                              // test-only: the same bits on both sides
    LSD_HD static double atan2(double y, double x) { return vpk_pmath::atan2(y, x); }
    LSD_HD static double sin(double x) { return vpk_pmath::sin(x); }
    LSD_HD static double cos(double x) { return vpk_pmath::cos(x); }
    LSD_HD static double exp(double x) { return vpk_pmath::exp(x); }
    LSD_HD static double log(double x) { return vpk_pmath::log(x); }
    LSD_HD static double log10(double x) { return vpk_pmath::log10(x); }
    LSD_HD static double pow(double x, double y) { return vpk_pmath::pow(x, y); }
    LSD_HD static double sinh(double x) { return vpk_pmath::sinh(x); }
};

// per-call constants, all made on the host
struct Params {
    double scale, prec, p, rho;
    int taps, half;            // Gaussian kernel: n = 1 + 2 h taps
};

// host-only: the constants of a call at `scale`, and the per-image ones
inline Params make_params(double scale) {
    Params q;
    q.scale = scale;
    q.prec = PI_L * ANG_TH / 180.0;
    q.p = ANG_TH / 180.0;
    q.rho = QUANT / sin(q.prec);
    const double sigma = scale < 1.0 ? SIGMA_SCALE / scale : SIGMA_SCALE;
    q.half = (int)ceil(sigma * sqrt(2.0 * 3.0 * log(10.0)));
    q.taps = 1 + 2 * q.half;
    return q;
}
inline void scaled_size(int width, int height, double scale, int& xs, int& ys) {
    if (scale != 1.0) {
        xs = (int)ceil(width * scale);
        ys = (int)ceil(height * scale);
    } else {
        xs = width;
        ys = height;
    }
}
inline double log_nt(int xs, int ys) { return 5.0 * (log10((double)xs) + log10((double)ys)) / 2.0 + log10(11.0); }
inline int min_reg_size(double logNT, double p) { return (int)(-logNT / log10(p)); }

// host-only: the normalised Gaussian kernel of every output coordinate 0..count-1 of both passes (the kernel of output
// coordinate i depends on i and the scale only): table[i * taps + k]
inline void gaussian_weights(double* table, int count, const Params& q) {
    const double sigma = q.scale < 1.0 ? SIGMA_SCALE / q.scale : SIGMA_SCALE;
    for (int c = 0; c < count; ++c) {
        const double xx = (double)c / q.scale;
        const int xc = (int)floor(xx + 0.5);
        const double mean = (double)q.half + xx - (double)xc;
        double* k = table + (size_t)c * q.taps;
        double sum = 0.0;
        for (int i = 0; i < q.taps; ++i) {
            const double v = ((double)i - mean) / sigma;
            k[i] = exp(-0.5 * v * v);
            sum += k[i];
        }
        if (sum >= 0.0)
            for (int i = 0; i < q.taps; ++i) k[i] /= sum;
    }
}

// ---- 1. Gaussian sub-sampling: one output sample of either pass ------------------------------------------------------
// src: `len` samples along the filtered axis, `stride` apart; c: output coordinate along it; w: its kernel (taps)
LSD_HD inline double sample(const double* src, int len, long long stride, int c, const double* w, const Params& q) {
    const double cc = (double)c / q.scale;
    const int xc = (int)floor(cc + 0.5);
    const int d2 = 2 * len;
    double sum = 0.0;
    for (int i = 0; i < q.taps; ++i) {
        int j = xc - q.half + i;
        while (j < 0) j += d2;
        while (j >= d2) j -= d2;
        if (j >= len) j = d2 - 1 - j;                          // symmetric boundary
        sum += src[(long long)j * stride] * w[i];
    }
    return sum;
}

// ---- 2. gradient, level-line angle, magnitude of pixel (x, y) of an xs x ys image ---------------------------------------
// returns the magnitude (0 on the last row / column); *angle = NOTDEF when it is at most rho
template <class M = Libm>
LSD_HD inline double gradient(const double* img, int xs, int ys, int x, int y, double rho, double* angle) {
    if (x >= xs - 1 || y >= ys - 1) {
        *angle = NOTDEF;
        return 0.0;
    }
    const long long adr = (long long)y * xs + x;
    const double com1 = img[adr + xs + 1] - img[adr];
    const double com2 = img[adr + 1] - img[adr + xs];
    const double gx = com1 + com2, gy = com1 - com2;
    const double norm = sqrt((gx * gx + gy * gy) / 4.0);
    *angle = norm <= rho ? NOTDEF : M::atan2(gx, -gy);              // level-line angle
    return norm;
}

// ---- 3. pseudo-ordering bin of a magnitude ---------------------------------------------------------------------------
LSD_HD inline int grad_bin(double norm, double max_grad) {
    int i = (int)(norm * (double)N_BINS / max_grad);
    if (i >= N_BINS) i = N_BINS - 1;
    if (i < 0) i = 0;                                            // (a NaN pixel: keeps the device's LDS index in range)
    return i;
}

// ---- helpers of the region stage ------------------------------------------------------------------------------------
LSD_HD inline double dist(double x1, double y1, double x2, double y2) {
    return sqrt((x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1));
}

LSD_HD inline bool double_equal(double a, double b) {
    if (a == b) return true;
    const double diff = fabs(a - b), aa = fabs(a), bb = fabs(b);
    double mx = aa > bb ? aa : bb;
    if (mx < DBL_MIN) mx = DBL_MIN;
    return diff / mx <= 100.0 * DBL_EPSILON;
}

LSD_HD inline bool isaligned_a(double a, double theta, double prec) {
    if (a == NOTDEF) return false;
    theta -= a;
    if (theta < 0.0) theta = -theta;
    if (theta > M_3_2_PI_L) {
        theta -= M_2__PI_L;
        if (theta < 0.0) theta = -theta;
    }
    return theta <= prec;
}

LSD_HD inline double angle_diff_signed(double a, double b) {
    a -= b;
    while (a <= -PI_L) a += M_2__PI_L;
    while (a > PI_L) a -= M_2__PI_L;
    return a;
}
LSD_HD inline double angle_diff(double a, double b) { return fabs(angle_diff_signed(a, b)); }

// ---- 7. NFA ---------------------------------------------------------------------------------------------------------
template <class M>
LSD_HD inline double log_gamma_lanczos(double x) {
    const double q[7] = {75122.6331530, 80916.6278952, 36308.2951477, 8687.24529705, 1168.92649479, 83.8676043424,
                         2.50662827511};
    double a = (x + 0.5) * M::log(x + 5.5) - (x + 5.5);
    double b = 0.0;
    for (int n = 0; n < 7; ++n) {
        a -= M::log(x + (double)n);
        b += q[n] * M::pow(x, (double)n);
    }
    return a + M::log(b);
}
template <class M>
LSD_HD inline double log_gamma_windschitl(double x) {
    return 0.918938533204673 + (x - 0.5) * M::log(x) - x +
           0.5 * x * M::log(x * M::sinh(1 / x) + 1 / (810.0 * M::pow(x, 6.0)));
}
template <class M>
LSD_HD inline double log_gamma(double x) { return x > 15.0 ? log_gamma_windschitl<M>(x) : log_gamma_lanczos<M>(x); }

template <class M = Libm>
LSD_HD inline double nfa(int n, int k, double p, double logNT) {
    const double tolerance = 0.1;
    if (n == 0 || k == 0) return -logNT;
    if (n == k) return -logNT - (double)n * M::log10(p);
    const double p_term = p / (1.0 - p);
    const double log1term = log_gamma<M>((double)n + 1.0) - log_gamma<M>((double)k + 1.0) -
                            log_gamma<M>((double)(n - k) + 1.0) + (double)k * M::log(p) + (double)(n - k) * M::log(1.0 - p);
    double term = M::exp(log1term);
    if (double_equal(term, 0.0)) {
        if ((double)k > (double)n * p) return -log1term / LN10_L - logNT;
        return -logNT;
    }
    double bin_tail = term;
    for (int i = k + 1; i <= n; ++i) {
        const double bin_term = (double)(n - i + 1) / (double)i;
        const double mult_term = bin_term * p_term;
        term *= mult_term;
        bin_tail += term;
        if (bin_term < 1.0) {
            const double err = term * ((1.0 - M::pow(mult_term, (double)(n - i + 1))) / (1.0 - mult_term) - 1.0);
            if (err < tolerance * fabs(-M::log10(bin_tail) - logNT) * bin_tail) break;
        }
    }
    return -M::log10(bin_tail) - logNT;
}

LSD_HD inline double inter_low(double x, double x1, double y1, double x2, double y2) {
    if (double_equal(x1, x2) && y1 < y2) return y1;
    if (double_equal(x1, x2) && y1 > y2) return y2;
    return y1 + (x - x1) * (y2 - y1) / (x2 - x1);
}
LSD_HD inline double inter_hi(double x, double x1, double y1, double x2, double y2) {
    if (double_equal(x1, x2) && y1 < y2) return y2;
    if (double_equal(x1, x2) && y1 > y2) return y1;
    return y1 + (x - x1) * (y2 - y1) / (x2 - x1);
}

// One image's region stage.  W is the wave the stage runs on: lane() / size() and the reductions sum_int(int),
// max_d(double), min_d(double) over its lanes (a one-lane wave on the host).  Every lane runs the same sequential code
// with the same values; loops split over lanes are marked.  M: the math policy.
template <class W, class M = Libm>
struct Region {
    const W& w;
    const double* angles;
    const double* modgrad;
    unsigned char* used;
    Pt* reg;
    int xs, ys;
    double logNT;

    LSD_HD double angle(int x, int y) const { return angles[(long long)y * xs + x]; }
    LSD_HD double grad(int x, int y) const { return modgrad[(long long)y * xs + x]; }
    LSD_HD unsigned char& use(int x, int y) const { return used[(long long)y * xs + x]; }

    // rect_nfa: LSD's rectangle iterator visits, column by column, x = ceil(vx[0]) .. (x <= vx[2]) and in each column
    // y = ceil(ys) .. (y <= ye), and counts the pixels inside the image; the columns are independent, so the lanes
    // take them in turn [split]
    LSD_HD double rect_nfa(const Rect& r) const {
        double vxr[4], vyr[4], vx[4], vy[4];
        vxr[0] = r.x1 - r.dy * r.width / 2.0; vyr[0] = r.y1 + r.dx * r.width / 2.0;
        vxr[1] = r.x2 - r.dy * r.width / 2.0; vyr[1] = r.y2 + r.dx * r.width / 2.0;
        vxr[2] = r.x2 + r.dy * r.width / 2.0; vyr[2] = r.y2 - r.dx * r.width / 2.0;
        vxr[3] = r.x1 + r.dy * r.width / 2.0; vyr[3] = r.y1 - r.dx * r.width / 2.0;
        int offset;
        if (r.x1 < r.x2 && r.y1 <= r.y2) offset = 0;
        else if (r.x1 >= r.x2 && r.y1 < r.y2) offset = 1;
        else if (r.x1 > r.x2 && r.y1 >= r.y2) offset = 2;
        else offset = 3;
        for (int n = 0; n < 4; ++n) {
            vx[n] = vxr[(offset + n) % 4];
            vy[n] = vyr[(offset + n) % 4];
        }
        int x0 = (int)ceil(vx[0]);
        if (x0 < 0) x0 = 0;
        int pts = 0, alg = 0;
        for (int x = x0 + w.lane(); x < xs && (double)x <= vx[2]; x += w.size()) {
            const double ys_ = (double)x < vx[3] ? inter_low((double)x, vx[0], vy[0], vx[3], vy[3])
                                                 : inter_low((double)x, vx[3], vy[3], vx[2], vy[2]);
            const double ye = (double)x < vx[1] ? inter_hi((double)x, vx[0], vy[0], vx[1], vy[1])
                                                : inter_hi((double)x, vx[1], vy[1], vx[2], vy[2]);
            int y = (int)ceil(ys_);
            if (y < 0) y = 0;
            for (; y < ys && (double)y <= ye; ++y) {
                ++pts;
                if (isaligned_a(angle(x, y), r.theta, r.prec)) ++alg;
            }
        }
        return nfa<M>(w.sum_int(pts), w.sum_int(alg), r.p, logNT);
    }

    // 4. region growing
    LSD_HD void region_grow(int x, int y, int& reg_size, double& reg_angle, double prec) const {
        reg_size = 1;
        reg[0] = Pt{x, y};
        reg_angle = angle(x, y);
        double sumdx = M::cos(reg_angle), sumdy = M::sin(reg_angle);
        use(x, y) = 1;
        for (int i = 0; i < reg_size; ++i) {
            const Pt c = reg[i];
            for (int xx = c.x - 1; xx <= c.x + 1; ++xx)
                for (int yy = c.y - 1; yy <= c.y + 1; ++yy)
                    if (xx >= 0 && yy >= 0 && xx < xs && yy < ys && use(xx, yy) != 1) {
                        const double a = angle(xx, yy);
                        if (!isaligned_a(a, reg_angle, prec)) continue;
                        use(xx, yy) = 1;
                        reg[reg_size] = Pt{xx, yy};
                        ++reg_size;
                        sumdx += M::cos(a);
                        sumdy += M::sin(a);
                        reg_angle = M::atan2(sumdy, sumdx);
                    }
        }
    }

    // 5. rectangle approximation
    LSD_HD double get_theta(int reg_size, double x, double y, double reg_angle, double prec) const {
        double Ixx = 0.0, Iyy = 0.0, Ixy = 0.0;
        for (int i = 0; i < reg_size; ++i) {
            const Pt c = reg[i];
            const double wt = grad(c.x, c.y);
            Ixx += ((double)c.y - y) * ((double)c.y - y) * wt;
            Iyy += ((double)c.x - x) * ((double)c.x - x) * wt;
            Ixy -= ((double)c.x - x) * ((double)c.y - y) * wt;
        }
        const double lambda = 0.5 * (Ixx + Iyy - sqrt((Ixx - Iyy) * (Ixx - Iyy) + 4.0 * Ixy * Ixy));
        double theta = fabs(Ixx) > fabs(Iyy) ? M::atan2(lambda - Ixx, Ixy) : M::atan2(Ixy, lambda - Iyy);
        if (angle_diff(theta, reg_angle) > prec) theta += PI_L;
        return theta;
    }

    LSD_HD void region2rect(int reg_size, double reg_angle, double prec, double p, Rect& rec) const {
        double x = 0.0, y = 0.0, sum = 0.0;
        for (int i = 0; i < reg_size; ++i) {
            const Pt c = reg[i];
            const double wt = grad(c.x, c.y);
            x += (double)c.x * wt;
            y += (double)c.y * wt;
            sum += wt;
        }
        x /= sum;
        y /= sum;
        const double theta = get_theta(reg_size, x, y, reg_angle, prec);
        const double dx = M::cos(theta), dy = M::sin(theta);
        double l_min = 0.0, l_max = 0.0, w_min = 0.0, w_max = 0.0;
        for (int i = w.lane(); i < reg_size; i += w.size()) {              // [split]: min / max are exact
            const Pt c = reg[i];
            const double l = ((double)c.x - x) * dx + ((double)c.y - y) * dy;
            const double wd = -((double)c.x - x) * dy + ((double)c.y - y) * dx;
            if (l > l_max) l_max = l;
            if (l < l_min) l_min = l;
            if (wd > w_max) w_max = wd;
            if (wd < w_min) w_min = wd;
        }
        l_max = w.max_d(l_max); l_min = w.min_d(l_min);
        w_max = w.max_d(w_max); w_min = w.min_d(w_min);
        rec.x1 = x + l_min * dx; rec.y1 = y + l_min * dy;
        rec.x2 = x + l_max * dx; rec.y2 = y + l_max * dy;
        rec.width = w_max - w_min;
        rec.x = x; rec.y = y; rec.theta = theta; rec.dx = dx; rec.dy = dy; rec.prec = prec; rec.p = p;
        if (rec.width < 1.0) rec.width = 1.0;
    }

    // 6. refinement
    LSD_HD bool reduce_region_radius(int& reg_size, double reg_angle, double prec, double p, Rect& rec) const {
        double density = (double)reg_size / (dist(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width);
        if (density >= DENSITY_TH) return true;
        const double xc = (double)reg[0].x, yc = (double)reg[0].y;
        const double rad1 = dist(xc, yc, rec.x1, rec.y1), rad2 = dist(xc, yc, rec.x2, rec.y2);
        double rad = rad1 > rad2 ? rad1 : rad2;
        while (density < DENSITY_TH) {
            rad *= 0.75;
            for (int i = 0; i < reg_size; ++i)
                if (dist(xc, yc, (double)reg[i].x, (double)reg[i].y) > rad) {
                    use(reg[i].x, reg[i].y) = 0;
                    reg[i] = reg[reg_size - 1];
                    --reg_size;
                    --i;
                }
            if (reg_size < 2) return false;
            region2rect(reg_size, reg_angle, prec, p, rec);
            density = (double)reg_size / (dist(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width);
        }
        return true;
    }

    LSD_HD bool refine(int& reg_size, double reg_angle, double prec, double p, Rect& rec) const {
        double density = (double)reg_size / (dist(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width);
        if (density >= DENSITY_TH) return true;
        const double xc = (double)reg[0].x, yc = (double)reg[0].y;
        const double ang_c = angle(reg[0].x, reg[0].y);
        double sum = 0.0, s_sum = 0.0;
        int n = 0;
        for (int i = 0; i < reg_size; ++i) {
            use(reg[i].x, reg[i].y) = 0;
            if (dist(xc, yc, (double)reg[i].x, (double)reg[i].y) < rec.width) {
                const double ang_d = angle_diff_signed(angle(reg[i].x, reg[i].y), ang_c);
                sum += ang_d;
                s_sum += ang_d * ang_d;
                ++n;
            }
        }
        const double mean_angle = sum / (double)n;
        const double tau = 2.0 * sqrt((s_sum - 2.0 * mean_angle * sum) / (double)n + mean_angle * mean_angle);
        region_grow(reg[0].x, reg[0].y, reg_size, reg_angle, tau);
        if (reg_size < 2) return false;
        region2rect(reg_size, reg_angle, prec, p, rec);
        density = (double)reg_size / (dist(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width);
        if (density < DENSITY_TH) return reduce_region_radius(reg_size, reg_angle, prec, p, rec);
        return true;
    }

    LSD_HD double rect_improve(Rect& rec) const {
        const double delta = 0.5, delta_2 = delta / 2.0;
        double log_nfa = rect_nfa(rec);
        if (log_nfa > LOG_EPS) return log_nfa;
        Rect r = rec;                                              // finer precisions
        for (int n = 0; n < 5; ++n) {
            r.p /= 2.0;
            r.prec = r.p * PI_L;
            const double v = rect_nfa(r);
            if (v > log_nfa) { log_nfa = v; rec = r; }
        }
        if (log_nfa > LOG_EPS) return log_nfa;
        r = rec;                                                   // narrower
        for (int n = 0; n < 5; ++n)
            if ((r.width - delta) >= 0.5) {
                r.width -= delta;
                const double v = rect_nfa(r);
                if (v > log_nfa) { rec = r; log_nfa = v; }
            }
        if (log_nfa > LOG_EPS) return log_nfa;
        r = rec;                                                   // one side of the rectangle
        for (int n = 0; n < 5; ++n)
            if ((r.width - delta) >= 0.5) {
                r.x1 += -r.dy * delta_2; r.y1 += r.dx * delta_2;
                r.x2 += -r.dy * delta_2; r.y2 += r.dx * delta_2;
                r.width -= delta;
                const double v = rect_nfa(r);
                if (v > log_nfa) { rec = r; log_nfa = v; }
            }
        if (log_nfa > LOG_EPS) return log_nfa;
        r = rec;                                                   // the other side
        for (int n = 0; n < 5; ++n)
            if ((r.width - delta) >= 0.5) {
                r.x1 -= -r.dy * delta_2; r.y1 -= r.dx * delta_2;
                r.x2 -= -r.dy * delta_2; r.y2 -= r.dx * delta_2;
                r.width -= delta;
                const double v = rect_nfa(r);
                if (v > log_nfa) { rec = r; log_nfa = v; }
            }
        if (log_nfa > LOG_EPS) return log_nfa;
        r = rec;                                                   // even finer precisions
        for (int n = 0; n < 5; ++n) {
            r.p /= 2.0;
            r.prec = r.p * PI_L;
            const double v = rect_nfa(r);
            if (v > log_nfa) { log_nfa = v; rec = r; }
        }
        return log_nfa;
    }

    // the seed loop over `n_order` seeds (packed y * xs + x, pseudo-ordered; seeds whose angle is NOTDEF may be left out:
    // the loop skips them).  Rows go to out (max_segments of 7 doubles; lane 0 writes); returns the full count, which may
    // exceed max_segments.
    LSD_HD int detect(const int* order, int n_order, const Params& q, int min_reg, double* out, int max_segments) const {
        int count = 0;
        for (int k = 0; k < n_order; ++k) {
            const int s = order[k];
            const int sx = s % xs, sy = s / xs;
            if (use(sx, sy) != 0 || angle(sx, sy) == NOTDEF) continue;
            int reg_size = 0;
            double reg_angle = 0.0;
            region_grow(sx, sy, reg_size, reg_angle, q.prec);
            if (reg_size < min_reg) continue;
            Rect rec;
            region2rect(reg_size, reg_angle, q.prec, q.p, rec);
            if (!refine(reg_size, reg_angle, q.prec, q.p, rec)) continue;
            const double log_nfa = rect_improve(rec);
            if (log_nfa <= LOG_EPS) continue;
            rec.x1 += 0.5; rec.y1 += 0.5; rec.x2 += 0.5; rec.y2 += 0.5;   // the gradient sits between the pixels of its mask
            if (q.scale != 1.0) {
                rec.x1 /= q.scale; rec.y1 /= q.scale; rec.x2 /= q.scale; rec.y2 /= q.scale;
                rec.width /= q.scale;
            }
            if (count < max_segments && w.lane() == 0) {
                double* o = out + 7 * (long long)count;
                o[0] = rec.x1; o[1] = rec.y1; o[2] = rec.x2; o[3] = rec.y2; o[4] = rec.width; o[5] = rec.p; o[6] = log_nfa;
            }
            ++count;
        }
        return count;
    }
};

}  // namespace vpk_lsd

#endif
