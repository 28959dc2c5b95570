// lsd_portable_math.hpp -- TEST-ONLY elementary functions of the line segment detector (lsd_device.hpp's `Portable`
// math policy): atan2, sin, cos, exp, log, log10, pow, sinh written with + - * /, comparisons and bit operations on the
// exponent only -- no libm call, no fma, no sqrt.  Every operation is a correctly rounded IEEE double operation, so a
// unit built with -ffp-contract=off gives the same bits on gfx950 and on x86-64.  That lets the GPU detector be pinned
// bit for bit against its host build (tests/test_gpu_lsd_exact.py); the product's kernels keep the device libm.
//
// Accuracy (tests/test_lsd_portable_math.py, against mpmath at 50 digits) on what the detector feeds them: atan2 on
// the whole plane, sin / cos for |x| <= 4 pi, exp down to the subnormal results, log / log10 on (0, 1e300], pow(x, n)
// for integer n >= 0, sinh(1 / x) for x > 15.  The method is the textbook one: Cody-Waite reduction with split
// constants, Taylor polynomials on the reduced range long enough that truncation stays below 2^-56, and double-double
// (Dekker) arithmetic where a rounding would otherwise be amplified.  Outside those domains the results are finite where
// the function is, deterministic and less accurate (sin / cos beyond |x| = 2^28 return 0 / 1).
#ifndef VPK_LSD_PORTABLE_MATH_HPP_
#define VPK_LSD_PORTABLE_MATH_HPP_

#include <stdint.h>

#ifdef __HIPCC__
#define LSD_PM_HD __host__ __device__
#else
#define LSD_PM_HD
#endif

namespace vpk_pmath {

LSD_PM_HD inline uint64_t bits(double x) {
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof(u));
    return u;
}
LSD_PM_HD inline double from_bits(uint64_t u) {
    double x;
    __builtin_memcpy(&x, &u, sizeof(x));
    return x;
}
LSD_PM_HD inline double pow2i(int k) { return from_bits((uint64_t)(k + 1023) << 52); }   // 2^k, -1022 <= k <= 1023
LSD_PM_HD inline double fabs_(double x) { return from_bits(bits(x) & 0x7fffffffffffffffull); }
LSD_PM_HD inline bool is_nan(double x) { return x != x; }
LSD_PM_HD inline double inf_() { return from_bits(0x7ff0000000000000ull); }
LSD_PM_HD inline double nan_() { return from_bits(0x7ff8000000000000ull); }

// ---- double-double helpers (exact error terms) ----------------------------------------------------------------------
LSD_PM_HD inline void fast_two_sum(double a, double b, double& s, double& e) {   // |a| >= |b|
    s = a + b;
    e = (a - s) + b;
}
LSD_PM_HD inline void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// Dekker's product: p + e = a * b exactly (Veltkamp split; both factors below 2^995 in magnitude, no underflow)
LSD_PM_HD inline void two_prod(double a, double b, double& p, double& e) {
    p = a * b;
    if (!(fabs_(a) < 0x1p995 && fabs_(b) < 0x1p995 && fabs_(p) <= 0x1.fffffffffffffp1023)) {
        e = 0.0;
        return;
    }
    const double ca = 134217729.0 * a, cb = 134217729.0 * b;
    const double ah = ca - (ca - a), al = a - ah;
    const double bh = cb - (cb - b), bl = b - bh;
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl;
}
LSD_PM_HD inline void dd_mul(double ah, double al, double bh, double bl, double& h, double& l) {
    double p, e;
    two_prod(ah, bh, p, e);
    e += ah * bl + al * bh;
    fast_two_sum(p, e, h, l);
    if (!(fabs_(h) <= 0x1.fffffffffffffp1023)) { h = p; l = 0.0; }
}

// round to nearest integer (ties away from zero) of |v| < 2^31
LSD_PM_HD inline int round_int(double v) { return (int)(v < 0.0 ? v - 0.5 : v + 0.5); }

// ---- exp ------------------------------------------------------------------------------------------------------------
// x = k ln2 + r, |r| <= ln2 / 2 (ln2 in two parts, k * LN2_HI exact); exp(r) by its Taylor series to r^14 / 14!
constexpr double LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33, INV_LN2 = 0x1.71547652b82fep+0;

LSD_PM_HD inline double exp(double x) {
    if (is_nan(x)) return x + x;
    if (x > 709.8) return inf_();
    if (x < -746.0) return 0.0;
    const int k = round_int(x * INV_LN2);
    const double hi = x - (double)k * LN2_HI;                 // exact
    const double lo = (double)k * LN2_LO;
    const double r = hi - lo;
    const double rc = (hi - r) - lo;                          // r + rc = hi - lo to double-double precision
    const double c[13] = {0x1.0000000000000p-1, 0x1.5555555555555p-3, 0x1.5555555555555p-5, 0x1.1111111111111p-7,
                          0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-13, 0x1.a01a01a01a01ap-16, 0x1.71de3a556c734p-19,
                          0x1.27e4fb7789f5cp-22, 0x1.ae64567f544e4p-26, 0x1.1eed8eff8d898p-29, 0x1.6124613a86d09p-33,
                          0x1.93974a8c07c9dp-37};         // 1 / n!, n = 2 .. 14
    double p = c[12];
    for (int i = 11; i >= 0; --i) p = p * r + c[i];
    const double q = r * r * p;                               // exp(r) - 1 - r
    const double y = 1.0 + (r + (q + rc * (1.0 + r)));
    if (k > 1023) return y * 2.0 * pow2i(k - 1);
    if (k >= -1021) return y * pow2i(k);
    return y * pow2i(k + 1000) * 0x1p-1000;                   // one rounding into the subnormals
}

// ---- log / log10 ----------------------------------------------------------------------------------------------------
// x = 2^e m, m in [sqrt(2)/2, sqrt(2)), f = m - 1 (exact), s = f / (2 + f):
// log(1 + f) = f - f^2/2 + s (f^2/2 + R(s^2)),  R(z) = sum 2 z^k / (2k + 1), k = 1 .. 12
LSD_PM_HD inline void log_parts(double x, int& e, double& f, double& s, double& hfsq, double& R) {
    uint64_t u = bits(x);
    e = 0;
    if ((u >> 52) == 0) {                                     // subnormal
        x *= 0x1p54;
        u = bits(x);
        e = -54;
    }
    e += (int)(u >> 52) - 1023;
    double m = from_bits((u & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
    if (m > 0x1.6a09e667f3bcdp+0) {
        m *= 0.5;
        ++e;
    }
    f = m - 1.0;
    s = f / (2.0 + f);
    const double z = s * s;
    const double c[12] = {0x1.5555555555555p-1, 0x1.999999999999ap-2, 0x1.2492492492492p-2, 0x1.c71c71c71c71cp-3,
                          0x1.745d1745d1746p-3, 0x1.3b13b13b13b14p-3, 0x1.1111111111111p-3, 0x1.e1e1e1e1e1e1ep-4,
                          0x1.af286bca1af28p-4, 0x1.8618618618618p-4, 0x1.642c8590b2164p-4, 0x1.47ae147ae147bp-4};
    double p = c[11];
    for (int i = 10; i >= 0; --i) p = p * z + c[i];
    R = z * p;
    hfsq = 0.5 * f * f;
}

LSD_PM_HD inline double log(double x) {
    if (is_nan(x) || x < 0.0) return nan_();
    if (x == 0.0) return -inf_();
    if (x == inf_()) return x;
    int e;
    double f, s, hfsq, R;
    log_parts(x, e, f, s, hfsq, R);
    const double de = (double)e;
    return de * LN2_HI + (f - (hfsq - (s * (hfsq + R) + de * LN2_LO)));
}

// log10 x = log x / ln 10 with log x in double-double: (e ln2 + log(1 + f)) * (INV_LN10 + its tail)
constexpr double INV_LN10_HI = 0x1.bcb7b1526e50ep-2, INV_LN10_LO = 0x1.95355baaafad3p-57;

LSD_PM_HD inline double log10(double x) {
    if (is_nan(x) || x < 0.0) return nan_();
    if (x == 0.0) return -inf_();
    if (x == inf_()) return x;
    int e;
    double f, s, hfsq, R;
    log_parts(x, e, f, s, hfsq, R);
    const double de = (double)e;
    // log(1 + f) = f_hi + f_lo with f - hfsq in two parts
    double a, b;
    two_sum(f, -hfsq, a, b);
    b += s * (hfsq + R);
    double lh, ll;
    two_sum(de * LN2_HI, a, lh, ll);                          // de * LN2_HI is exact
    ll += b + de * LN2_LO;
    fast_two_sum(lh, ll, lh, ll);
    double h, l;
    dd_mul(lh, ll, INV_LN10_HI, INV_LN10_LO, h, l);
    return h + l;
}

// ---- sin / cos ------------------------------------------------------------------------------------------------------
// x = k pi/2 + r, |r| <= pi/4, with pi/2 in three parts (k * PIO2_1 and k * PIO2_2 exact for |k| < 2^20) and r kept as
// a double-double r_hi + r_lo
constexpr double PIO2_1 = 0x1.921fb54400000p+0, PIO2_2 = 0x1.0b4611a600000p-34, PIO2_3 = 0x1.3198a2e037073p-69;
constexpr double TWO_OVER_PI = 0x1.45f306dc9c883p-1;

LSD_PM_HD inline void trig_reduce(double x, int& k, double& rh, double& rl) {
    k = round_int(x * TWO_OVER_PI);
    const double dk = (double)k;
    const double r1 = x - dk * PIO2_1;                        // exact near k pi/2
    double s, e;
    two_sum(r1, -(dk * PIO2_2), s, e);
    e -= dk * PIO2_3;
    two_sum(s, e, rh, rl);
}
// sin(h + l) = h + (h z S(z) + l cos h), z = h^2, S = sum (-1)^n z^(n-1) / (2n + 1)!, n = 1 .. 10
LSD_PM_HD inline double sin_k(double h, double l) {
    const double z = h * h;
    const double c[10] = {-0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19,
                          -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49,
                          -0x1.2f49b46814157p-57, 0x1.71b8ef6dcf572p-66};
    double p = c[9];
    for (int i = 8; i >= 0; --i) p = p * z + c[i];
    return h + (h * z * p + l * (1.0 - 0.5 * z));
}
// cos(h + l) = 1 - h^2/2 + h^4 C(h^2) - l h, with h^2 exact in two parts and 1 - h^2/2 compensated
LSD_PM_HD inline double cos_k(double h, double l) {
    double zh, zl;
    two_prod(h, h, zh, zl);
    const double hz = 0.5 * zh;
    const double w = 1.0 - hz;
    const double corr = ((1.0 - w) - hz) - 0.5 * zl;
    const double c[10] = {0x1.5555555555555p-5, -0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-16, -0x1.27e4fb7789f5cp-22,
                          0x1.1eed8eff8d898p-29, -0x1.93974a8c07c9dp-37, 0x1.ae7f3e733b81fp-45, -0x1.6827863b97d97p-53,
                          0x1.e542ba4020225p-62, -0x1.0ce396db7f853p-70};   // (-1)^n / (2n)!, n = 2 .. 11
    double p = c[9];
    for (int i = 8; i >= 0; --i) p = p * zh + c[i];
    return w + (corr + (zh * zh * p - h * l));
}

LSD_PM_HD inline double sin(double x) {
    if (is_nan(x) || fabs_(x) == inf_()) return nan_();
    if (!(fabs_(x) <= 0x1p28)) return 0.0;
    int k;
    double h, l;
    trig_reduce(x, k, h, l);
    switch (k & 3) {
        case 0: return sin_k(h, l);
        case 1: return cos_k(h, l);
        case 2: return -sin_k(h, l);
        default: return -cos_k(h, l);
    }
}
LSD_PM_HD inline double cos(double x) {
    if (is_nan(x) || fabs_(x) == inf_()) return nan_();
    if (!(fabs_(x) <= 0x1p28)) return 1.0;
    int k;
    double h, l;
    trig_reduce(x, k, h, l);
    switch (k & 3) {
        case 0: return cos_k(h, l);
        case 1: return -sin_k(h, l);
        case 2: return -cos_k(h, l);
        default: return sin_k(h, l);
    }
}

// ---- atan2 ----------------------------------------------------------------------------------------------------------
// atan t for 0 <= t <= 1 as a double-double: t <= 3/16 by the series; else t = c + ..., c = j / 8, with
// atan t = atan c + atan u, u = (t - c) / (1 + t c), |u| < 1/16
constexpr double PIO2_HI = 0x1.921fb54442d18p+0, PIO2_LO = 0x1.1a62633145c07p-54;
constexpr double PI_HI = 0x1.921fb54442d18p+1, PI_LO = 0x1.1a62633145c07p-53;

LSD_PM_HD inline double atan_series(double u) {               // atan(u) - u, |u| <= 3/16
    const double c[12] = {-0x1.5555555555555p-2, 0x1.999999999999ap-3, -0x1.2492492492492p-3, 0x1.c71c71c71c71cp-4,
                          -0x1.745d1745d1746p-4, 0x1.3b13b13b13b14p-4, -0x1.1111111111111p-4, 0x1.e1e1e1e1e1e1ep-5,
                          -0x1.af286bca1af28p-5, 0x1.8618618618618p-5, -0x1.642c8590b2164p-5, 0x1.47ae147ae147bp-5};
    const double z = u * u;
    double p = c[11];
    for (int i = 10; i >= 0; --i) p = p * z + c[i];
    return u * z * p;
}
LSD_PM_HD inline void atan01(double t, double& h, double& l) {
    if (t <= 0.1875) {
        fast_two_sum(t, atan_series(t), h, l);
        return;
    }
    const double hi[7] = {0x1.f5b75f92c80ddp-3, 0x1.6f61941e4def1p-2, 0x1.dac670561bb4fp-2, 0x1.1e00babdefeb4p-1,
                          0x1.4978fa3269ee1p-1, 0x1.700a7c5784634p-1, 0x1.921fb54442d18p-1};
    const double lo[7] = {0x1.8ab6e3cf7afbdp-57, -0x1.c63aae6f6e918p-56, 0x1.a2b7f222f65e2p-56, -0x1.928df287a668fp-58,
                          0x1.2419a87f2a458p-56, -0x1.8c34d25aadef6p-56, 0x1.1a62633145c07p-55};   // atan(j / 8), j = 2 .. 8
    const int j = round_int(8.0 * t);
    const double c = 0.125 * (double)j;
    const double u = (t - c) / (1.0 + t * c);                 // t - c exact
    fast_two_sum(hi[j - 2], lo[j - 2] + (u + atan_series(u)), h, l);
}

LSD_PM_HD inline double atan2(double y, double x) {
    if (is_nan(x) || is_nan(y)) return x + y;
    const bool neg_y = (bits(y) >> 63) != 0, neg_x = (bits(x) >> 63) != 0;
    const double ax = fabs_(x), ay = fabs_(y);
    double h, l;
    if (ax == inf_() && ay == inf_()) {
        h = neg_x ? 0x1.2d97c7f3321d2p+1 : 0x1.921fb54442d18p-1;     // 3 pi / 4, pi / 4
        return neg_y ? -h : h;
    }
    if (ay == 0.0) {
        h = neg_x ? PI_HI : 0.0;                              // atan2(+-0, +-0) and atan2(+-0, x): C99 Annex F
        return neg_y ? -h : h;
    }
    if (ay <= ax) {
        atan01(ay / ax, h, l);
    } else {
        double a, b, s, e;
        atan01(ax / ay, a, b);
        two_sum(PIO2_HI, -a, s, e);
        fast_two_sum(s, e + (PIO2_LO - b), h, l);
    }
    if (neg_x) {
        double s, e;
        two_sum(PI_HI, -h, s, e);
        fast_two_sum(s, e + (PI_LO - l), h, l);
    }
    const double r = h + l;
    return neg_y ? -r : r;
}

// ---- pow ------------------------------------------------------------------------------------------------------------
// x^n for an integer n, |n| < 2^31: binary powering in double-double (relative error ~ log2(n) 2^-104 before the final
// rounding).  Other exponents: exp(y log x), deterministic but not faithful (the detector never uses them).
LSD_PM_HD inline double pow(double x, double y) {
    if (y == 0.0) return 1.0;
    if (is_nan(x) || is_nan(y)) return x + y;
    if (fabs_(y) < 0x1p31 && (double)(int)y == y) {
        int n = (int)y;
        const bool inv = n < 0;
        if (inv) n = -n;
        double rh = 1.0, rl = 0.0, bh = x, bl = 0.0;
        while (true) {
            if (n & 1) dd_mul(rh, rl, bh, bl, rh, rl);
            n >>= 1;
            if (!n) break;
            dd_mul(bh, bl, bh, bl, bh, bl);
        }
        const double r = rh + rl;
        return inv ? 1.0 / r : r;
    }
    if (x > 0.0) return exp(y * log(x));
    if (x == 0.0) return y > 0.0 ? 0.0 : inf_();
    return nan_();
}

// ---- sinh -----------------------------------------------------------------------------------------------------------
// |x| < 1: x + x z P(z), z = x^2, P = sum z^(n-1) / (2n + 1)!, n = 1 .. 13; beyond: (e^x - e^-x) / 2
LSD_PM_HD inline double sinh(double x) {
    if (is_nan(x)) return x + x;
    const double ax = fabs_(x);
    if (ax < 1.0) {
        const double c[13] = {0x1.5555555555555p-3, 0x1.1111111111111p-7, 0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19,
                              0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, 0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49,
                              0x1.2f49b46814157p-57, 0x1.71b8ef6dcf572p-66, 0x1.761b41316381ap-75, 0x1.3f3ccdd165fa9p-84,
                              0x1.d1ab1c2dccea3p-94};
        const double z = x * x;
        double p = c[12];
        for (int i = 11; i >= 0; --i) p = p * z + c[i];
        return x + x * z * p;
    }
    const double E = exp(ax);
    const double r = 0.5 * (E - 1.0 / E);
    return x < 0.0 ? -r : r;
}

}  // namespace vpk_pmath

#endif
