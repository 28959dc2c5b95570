// trainset_device.hpp -- the per-element rules of the device-resident training set (vpk_trainset.hip), for device and host.
//
// The set stands where train/train_val.prototxt:1-62 has its two LMDB Data layers: a training example is an image's
// homogeneous lines (the sphere raster reads nothing else, and a line only up to scale) and its ground-truth vanishing
// points (the label map).  An augmentation of the image plane is therefore one 3 x 3 map of the lines and of the VPs, and
// its ground truth is exact by construction.  Everything here is fp64, every product, sum and difference rounded on its
// own (the unit is built with -ffp-contract=off); tests/hostsim/sim_trainset.cpp compiles these same functions with g++.
#ifndef VPK_TRAINSET_DEVICE_HPP_
#define VPK_TRAINSET_DEVICE_HPP_

#include <math.h>
#include <stdint.h>

#include "train_device.hpp"

#if defined(__HIPCC__)
#define VPK_TRAINSET_FN __host__ __device__ inline
#else
#define VPK_TRAINSET_FN inline
#endif

namespace vpk_trainset {

constexpr uint32_t DRAW_LAYER = 0x41;      // the `layer` word of the augmentation's draws (the dropout masks use 6 and 7)
constexpr uint32_t ORDER_LAYER = 0x53;     // of an epoch's shuffle keys
constexpr int MAX_GRID = 64;               // gh, gw of a label map: 1..64
constexpr int64_t MAX_MEAN_IMAGES = 4294967295ll / 255;   // 255 n fits a uint32 sum: 16 843 009 images

// ---- counter-based draws ------------------------------------------------------------------------------------------------
// Beside the dropout masks of train_device.hpp and with their hash: draw k of batch slot b at an iteration is
//   key = mask_key(seed, iteration, 0x41, b);   u_k = (mix64(key ^ k) >> 11) * 2^-53   in [0, 1)
// a pure function of (seed, iteration, b, k) and of nothing else.  An epoch's shuffle orders the examples by
//   mix64(mask_key(seed, epoch, 0x53, 0) ^ i),   ties (none in practice) by i.
VPK_TRAINSET_FN uint64_t draw_key(uint64_t seed, uint64_t iteration, uint32_t b) {
    return vpk_train::mask_key(seed, iteration, DRAW_LAYER, b);
}

VPK_TRAINSET_FN double draw(uint64_t key, uint64_t k) {
    return (double)(vpk_train::mix64(key ^ k) >> 11) * 1.1102230246251565e-16;   // 2^-53: both factors and the product exact
}

VPK_TRAINSET_FN uint64_t order_key(uint64_t seed, uint64_t epoch, uint64_t i) {
    return vpk_train::mix64(vpk_train::mask_key(seed, epoch, ORDER_LAYER, 0) ^ i);
}

// ---- the affine map H = [[h00, h01, h02], [h10, h11, h12], [0, 0, 1]], given as h[6] ----------------------------------------
VPK_TRAINSET_FN double affine_det(const double* h) { return h[0] * h[4] - h[1] * h[3]; }

VPK_TRAINSET_FN bool affine_valid(const double* h) {
    for (int i = 0; i < 6; ++i)
        if (!(fabs(h[i]) <= 1.7976931348623157e308)) return false;    // NaN and both infinities
    const double det = affine_det(h);
    return det != 0.0 && fabs(det) <= 1.7976931348623157e308;
}

// det * H^-T l: the line through the images of l's points, up to scale
VPK_TRAINSET_FN void transform_line(const double* h, const double* l, double* m) {
    const double det = h[0] * h[4] - h[1] * h[3];
    const double mx = h[4] * l[0] - h[3] * l[1];
    const double my = h[0] * l[1] - h[1] * l[0];
    const double mz = det * l[2] - (h[2] * mx + h[5] * my);
    m[0] = mx;
    m[1] = my;
    m[2] = mz;
}

// H v
VPK_TRAINSET_FN void transform_vp(const double* h, const double* v, double* w) {
    const double wx = (h[0] * v[0] + h[1] * v[1]) + h[2] * v[2];
    const double wy = (h[3] * v[0] + h[4] * v[1]) + h[5] * v[2];
    w[0] = wx;
    w[1] = wy;
    w[2] = v[2];
}

// ---- the label cell of a VP: train.label_maps' rule on a (gh, gw) grid -------------------------------------------------------
// normalise, flip into z >= 0, coordinate_conversion.point_to_angle and angle_to_index with their order of operations,
// floor(idx + 0.5) on both axes.  Returns a * gw + b, or -1 for a VP that is dropped: a zero or non-finite vector, a
// non-finite index (0 / 0 at the poles of the sphere) or a cell outside the map.
VPK_TRAINSET_FN bool finite64(double x) { return fabs(x) <= 1.7976931348623157e308; }

VPK_TRAINSET_FN int label_cell(const double* v, int gh, int gw) {
    if (!finite64(v[0]) || !finite64(v[1]) || !finite64(v[2])) return -1;
    const double norm = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(norm > 0.0)) return -1;
    double px = v[0] / norm, py = v[1] / norm, pz = v[2] / norm;
    if (pz < 0.0) {
        px = -px;
        py = -py;
    }
    const double beta = asin(py);
    double inner = px / cos(beta);
    inner = inner > 1.0 ? 1.0 : inner;          // np.minimum / np.maximum: a NaN stays a NaN
    inner = inner < -1.0 ? -1.0 : inner;
    const double alpha = asin(inner);
    const double pi = 3.141592653589793;
    const double a = ((alpha / pi + 0.5) - 0.5 / (double)gh) * (double)gh;
    const double b = ((beta / pi + 0.5) - 0.5 / (double)gw) * (double)gw;
    if (!finite64(a) || !finite64(b)) return -1;
    const double fa = floor(a + 0.5), fb = floor(b + 0.5);
    if (!(fa >= 0.0 && fa < (double)gh && fb >= 0.0 && fb < (double)gw)) return -1;
    return (int)fa * gw + (int)fb;
}

// the batch slot of output element t: the b with off[b] <= t < off[b + 1] in a rising prefix off[0..B] (empty slots skipped)
VPK_TRAINSET_FN int slot_of(const long long* off, int B, long long t) {
    int lo = 0, hi = B;                          // off[lo] <= t < off[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace vpk_trainset

#endif
