// score_device.hpp -- the scoring of a benchmark run (vpk_score.hip): the horizon error of an image against its ground truth
// (benchmark.py:245-253) and the area under the cumulative error curve (auc.py:5-37).  Compiled by hipcc into the kernels of
// vpk_score.hip and -- unmodified, with SC_HD empty -- by g++ into the test-only host build tests/hostsim/sim_score.cpp, which
// checks it against NumPy.  Both builds use -ffp-contract=off: every operation below rounds on its own.
//
// 1. Error.  thP = np.cross(trueHorizon, [+-1, 0, 1]) as NumPy evaluates a 3-vector cross product (c0 = a1 b2 - a2 b1,
//    c1 = a2 b0 - a0 b2, c2 = a0 b1 - a1 b0: two rounded products, one rounded difference), thP / thP[2], then
//    maximum(|hP1[1] - thP1[1]|, |hP2[1] - thP2[1]|) / 2 * scale * 1.0 / height left to right; maximum hands a NaN on.
// 2. AUC.  The errors in np.sort's order (ascending, NaN last) come from a rank by counting: error i goes to the position
//    given by the number of errors that precede it, equal errors told apart by their index, so the ranks are a permutation.
//    The curve is (err[i], (i + 1) / n); its value at the cutoff is auc.py:20-28's `mid`, the tail point (cutoff, 1 or mid)
//    comes after every data point with err <= cutoff (np.argsort(kind="stable")), and the area is the trapezoid sum over
//    the k data points with err <= cutoff plus the tail point, divided by the cutoff.  The sum is made by AUC_THREADS
//    strided partial sums and a fixed tree over them, so the same input gives the same bits wherever it runs.
// Citations are file:line under the reference tree.
#ifndef VPK_SCORE_DEVICE_HPP_
#define VPK_SCORE_DEVICE_HPP_

#include <stdint.h>

#ifdef __HIPCC__
#define SC_HD __host__ __device__
#else
#define SC_HD
#endif

namespace vpk_score {

constexpr int AUC_MAX_N = 65536;   // errors per vpk_auc call
constexpr int AUC_THREADS = 256;   // partial sums of the trapezoid sum; a power of two

// ---- 1. error ------------------------------------------------------------------------------------------------------
// np.cross(a, b) for two 3-vectors
SC_HD inline void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// np.maximum(a, b) on doubles
SC_HD inline double np_maximum(double a, double b) { return (a >= b || a != a) ? a : b; }
// benchmark.py:245-253 from hP1[1], hP2[1], the true horizon th[3] and the size of the image file
SC_HD inline double horizon_error(double hp1y, double hp2y, const double* th, int w, int h) {
    const double scale = (double)(w > h ? w : h);          // np.maximum(imageWidth, imageHeight), :137
    const double e1[3] = {1.0, 0.0, 1.0}, e2[3] = {-1.0, 0.0, 1.0};
    double t1[3], t2[3];
    cross3(th, e1, t1);                                    // :248
    cross3(th, e2, t2);                                    // :249
    const double t1y = t1[1] / t1[2], t2y = t2[1] / t2[2]; // :250-251
    const double m = np_maximum(__builtin_fabs(hp1y - t1y), __builtin_fabs(hp2y - t2y));
    return m / 2.0 * scale * 1.0 / (double)h;              // :253
}

// ---- 2. AUC --------------------------------------------------------------------------------------------------------
// does error j come before error i in np.sort's order, made a strict order by the index?
SC_HD inline bool err_precedes(double ej, int j, double ei, int i) {
    const bool nj = ej != ej, ni = ei != ei;
    if (ni) return !nj || j < i;                           // NaN last; among NaNs the lower index first
    if (nj) return false;
    return ej < ei || (ej == ei && j < i);
}
// pts[i, 1] = (np.arange(n) + 1) * 1.0 / n  (auc.py:12)
SC_HD inline double auc_frac(int i, int n) { return (double)(i + 1) * 1.0 / (double)n; }
// what "thread" t of T sees of the sorted errors s: how many of s[t], s[t + T], ... are <= cutoff, and the largest i among
// them with s[i - 1] < cutoff < s[i] (auc.py:20-28's test; 0: none -- i = 0 is never a crossing)
SC_HD inline void auc_scan(const double* s, int n, double cutoff, int t, int T, int* below, int* crossing) {
    int k = 0, c = 0;
    for (int i = t; i < n; i += T) {
        k += s[i] <= cutoff ? 1 : 0;
        if (i >= 1 && s[i - 1] < cutoff && cutoff < s[i]) c = i;
    }
    *below = k;
    *crossing = c;
}
// the tail point's y: 1 when the largest error is below the cutoff (auc.py:30), else mid = 1, or the interpolation at the
// last crossing (auc.py:27)
SC_HD inline double auc_tail_y(const double* s, int n, double cutoff, int crossing) {
    if (s[n - 1] < cutoff) return 1.0;
    if (crossing < 1) return 1.0;
    const int i = crossing;
    return (s[i - 1] * auc_frac(i - 1, n) + s[i] * auc_frac(i, n)) / (s[i] + s[i - 1]);
}
// term j of the trapezoid sum over the k data points with s <= cutoff and the tail point: d * (y[j + 1] + y[j]) / 2.0
SC_HD inline double auc_term(const double* s, int n, int k, double cutoff, double tail_y, int j) {
    if (j < k - 1) return (s[j + 1] - s[j]) * (auc_frac(j + 1, n) + auc_frac(j, n)) / 2.0;
    return (cutoff - s[j]) * (tail_y + auc_frac(j, n)) / 2.0;
}
// the terms t, t + T, ... < k in ascending order
SC_HD inline double auc_partial(const double* s, int n, int k, double cutoff, double tail_y, int t, int T) {
    double sum = 0.0;
    for (int j = t; j < k; j += T) sum = sum + auc_term(s, n, k, cutoff, tail_y, j);
    return sum;
}
// the fixed tree over T partial sums (T a power of two), as the workgroup of vpk_score.hip walks it; the sum ends in p[0]
SC_HD inline void auc_tree(double* p, int T) {
    for (int half = T / 2; half > 0; half /= 2)
        for (int t = 0; t < half; ++t) p[t] = p[t] + p[t + half];
}

}  // namespace vpk_score

#endif
