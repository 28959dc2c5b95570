// image_device.hpp -- the arithmetic of the GPU image front end (vpk_frontend.hip): decoded uint8 images -> the fp64 grey
// levels the line segment detector reads, and the detector's rows -> the reference's normalised segments and homogeneous
// lines.  Compiled by hipcc into the kernels of vpk_frontend.hip and -- unmodified, with IMG_HD empty -- by g++ into the
// test-only host build tests/hostsim/sim_frontend.cpp, which checks it against Pillow and numpy.
//
// 1. Fit-resize (frontend.resize_to_fit: Pillow's Image.resize(..., LANCZOS) on uint8 data).  Separable, in fixed point:
//    the weights of every output index of an axis are made on the HOST by lanczos_coeffs below (glibc sin, M_PI, the
//    normalisation and the rounding to 22 fraction bits of Pillow's precompute_coeffs / normalize_coeffs_8bpc); the
//    passes are integer sums (resample_px).  The horizontal pass runs first and is clipped to uint8; the vertical pass
//    reads that intermediate.  A pass whose size is unchanged is skipped.
// 2. Grey levels (frontend._detector_input(frontend.rgb2gray(x))): (((r/255)*0.2125 + (g/255)*0.7154) + (b/255)*0.0721) * 255,
//    left to right and without contraction (the translation unit is built with -ffp-contract=off); (g/255) * 255 for one
//    channel.  rgb2gray's np.dot rounds its sum in a BLAS-dependent order, so this is its value to within a few ulp.
// 3. Rows -> lines (frontend.detect_lsd_lines + homogeneous_lines, evaluation.py:161-168 / :227-251): the same fp64
//    operations as the numpy code, each rounded on its own.
#ifndef VPK_IMAGE_DEVICE_HPP_
#define VPK_IMAGE_DEVICE_HPP_

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define IMG_HD __host__ __device__
#else
#define IMG_HD
#endif

namespace vpk_img {

constexpr int PRECISION_BITS = 22;          // Pillow's 8-bit resampling: 32 - 8 - 2
constexpr double LANCZOS_SUPPORT = 3.0;

// ---- 1. Lanczos weights (host only) ---------------------------------------------------------------------------------
inline double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
inline double lanczos_filter(double x) {
    if (-LANCZOS_SUPPORT <= x && x < LANCZOS_SUPPORT) return sinc_filter(x) * sinc_filter(x / 3);
    return 0.0;
}
// taps per output index for a resize of in_size -> out_size samples
inline int lanczos_ksize(int in_size, int out_size) {
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(LANCZOS_SUPPORT * filterscale) * 2 + 1;
}
// bounds[2 i] = first input index of output i, bounds[2 i + 1] = how many; coeffs[i * ksize + k]: its fixed-point weights
// (zero past the count).  scratch: ksize doubles.
inline void lanczos_coeffs(int in_size, int out_size, int ksize, int32_t* bounds, int32_t* coeffs, double* scratch) {
    const double scale = (double)in_size / out_size;     // Pillow: (in1 - in0) of the float box (0, in_size), exact
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = LANCZOS_SUPPORT * filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            const double w = lanczos_filter((x + xmin - center + 0.5) * ss);
            scratch[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) scratch[x] /= ww;
        int32_t* k = coeffs + (long long)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            if (x >= xmax) {
                k[x] = 0;
                continue;
            }
            const double v = scratch[x];
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

// ---- 1. one resampled sample: `n` inputs `stride` bytes apart from src, weights k -----------------------------------
IMG_HD inline uint8_t resample_px(const uint8_t* src, long long stride, int n, const int32_t* k) {
    int32_t ss = 1 << (PRECISION_BITS - 1);
    for (int x = 0; x < n; ++x) ss += (int32_t)src[(long long)x * stride] * k[x];
    if (ss <= 0) return 0;
    if (ss >= (256 << PRECISION_BITS)) return 255;               // Pillow's clip8
    return (uint8_t)(ss >> PRECISION_BITS);
}

// ---- 2. grey level of one pixel: the image frontend.detect_lsd_lines hands to the detector --------------------------
IMG_HD inline double grey_rgb(uint8_t r, uint8_t g, uint8_t b) {
    const double v = ((r / 255.0) * 0.2125 + (g / 255.0) * 0.7154) + (b / 255.0) * 0.0721;
    return v * 255;
}
IMG_HD inline double grey_l(uint8_t g) { return (g / 255.0) * 255; }

// ---- 3. one detector row (x1, y1, x2, y2, width, p, -log10(NFA)) of a w x h image -> lp (4), l (3) ---------------------
IMG_HD inline void row_to_line(const double* row, int w, int h, double* lp, double* l) {
    const double cw = w / 2.0, ch = h / 2.0;
    const double s = (w > h ? w : h) / 2.0;
    const double x1 = (row[0] - cw) / s, x2 = (row[2] - cw) / s;
    const double y1 = -((row[1] - ch) / s), y2 = -((row[3] - ch) / s);
    lp[0] = x1;
    lp[1] = y1;
    lp[2] = x2;
    lp[3] = y2;
    // np.cross((x1, y1, 1), (x2, y2, 1)): (y1 * 1 - 1 * y2, 1 * x2 - x1 * 1, x1 * y2 - y1 * x2)
    l[0] = y1 - y2;
    l[1] = x2 - x1;
    const double a = x1 * y2, b = y1 * x2;
    l[2] = a - b;
}

}  // namespace vpk_img

#endif
