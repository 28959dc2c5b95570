// detect_device.hpp -- the two small steps between the EM's VP sets and a detector's results (vpk_detect.hip): the order
// of an image's best VPs, and the conversion of normalised coordinates to pixels.  Compiled by hipcc into the kernels of
// vpk_detect.hip and -- unmodified, with DET_HD empty -- by g++ into the test-only host build tests/hostsim/sim_detect.cpp,
// which checks it against NumPy.  Both builds use -ffp-contract=off: every operation below rounds on its own.
//
// 1. Order (calc_horizon.py:34-36: np.argsort(counts)[::-1][:maxbest]).  The rule is np.argsort(counts, kind="stable")[::-1]:
//    descending counts; among equal counts the HIGHER index first; a NaN count ranks above every number, and among NaNs
//    the higher index comes first.  A VP's rank is the number of VPs that precede it, so no sort is needed.
// 2. Pixels (example.py:66-76, the inverse of detect_lsd_lines' normalisation, evaluation.py:240-249): with
//    scale = max(w, h),  x_px = x * scale / 2.0 + w / 2.0,  y_px = -y * scale / 2.0 + h / 2.0, left to right in fp64.
// Citations are file:line under the reference tree.
#ifndef VPK_DETECT_DEVICE_HPP_
#define VPK_DETECT_DEVICE_HPP_

#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define DET_HD __host__ __device__
#else
#define DET_HD
#endif

namespace vpk_det {

constexpr int MAX_VP = 64;     // VPs per image, and the most a caller may ask the order of

// ---- 1. order ------------------------------------------------------------------------------------------------------
// does VP j (count cj) come before VP i (count ci) in np.argsort(counts, kind="stable")[::-1]?  (j != i)
DET_HD inline bool vp_precedes(double cj, int j, double ci, int i) {
    const bool nj = cj != cj, ni = ci != ci;
    if (nj || ni) return nj && (!ni || j > i);          // NaN above every number; among NaNs the higher index first
    return cj > ci || (cj == ci && j > i);
}
// position of VP i among the M VPs with counts c[0..M)
DET_HD inline int vp_rank(const double* c, int M, int i) {
    const double ci = c[i];
    int rank = 0;
    for (int j = 0; j < M; ++j) rank += (j != i && vp_precedes(c[j], j, ci, i)) ? 1 : 0;
    return rank;
}
// num_vp as horizon_kernel clamps it (vpk_horizon.hip)
DET_HD inline int clamp_num_vp(int M, int max_vp) { return M < 0 ? 0 : (M > max_vp ? max_vp : M); }

// ---- 2. pixels -----------------------------------------------------------------------------------------------------
DET_HD inline double quiet_nan() {                      // np.nan's bits
    const uint64_t bits = 0x7ff8000000000000ull;
    double v;
    memcpy(&v, &bits, sizeof(v));
    return v;
}
// (x, y) normalised -> pixels of a w x h image
DET_HD inline void point_to_px(double x, double y, int w, int h, double* out) {
    const double scale = (double)(w > h ? w : h);
    out[0] = x * scale / 2.0 + (double)w / 2.0;
    out[1] = -y * scale / 2.0 + (double)h / 2.0;
}
// one segment (x1, y1, x2, y2)
DET_HD inline void segment_to_px(const double* s, int w, int h, double* out) {
    point_to_px(s[0], s[1], w, h, out);
    point_to_px(s[2], s[3], w, h, out + 2);
}
// one homogeneous VP: v[0] / v[2], v[1] / v[2] first; a VP at infinity gives what IEEE gives
DET_HD inline void vp_to_px(const double* v, int w, int h, double* out) {
    point_to_px(v[0] / v[2], v[1] / v[2], w, h, out);
}

}  // namespace vpk_det

#endif
