// convtrain_device.hpp -- the per-element rules of the conv stack's training step (vpk_convtrain.hip), for device and host.
//
// The stack is train/train_val.prototxt:66-288: Convolution (+ ReLU), LRN across channels and MAX pooling with Caffe's
// semantics.  Here are the shape rules, the pooling window and argmax, the LRN's forward and backward of one element, and
// the three index maps that turn a convolution's forward, data gradient and weight gradient into one product
//     C[m][n] = sum_r A(m, r) B(r, n)
// whose operands a kernel gathers element by element (gemm_a / gemm_b) and whose results it scatters (gemm_store).
// Everything is float32; tests/hostsim/sim_convtrain.cpp compiles these same functions with g++.
#ifndef VPK_CONVTRAIN_DEVICE_HPP_
#define VPK_CONVTRAIN_DEVICE_HPP_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VPK_CT_FN __host__ __device__ inline
#else
#define VPK_CT_FN inline
#endif

namespace vpk_convtrain {

// ---- shapes -------------------------------------------------------------------------------------------------------------
VPK_CT_FN int conv_out_size(int in, int K, int stride, int pad) {
    const int span = in + 2 * pad - K;
    return span < 0 ? 0 : span / stride + 1;
}

// Caffe's pooling layer without padding: ceil((in - K) / stride) + 1; the last window may be clipped, never empty: one
// that would start past the plane (K < stride) is dropped, as Caffe drops it
VPK_CT_FN int pool_out_size(int in, int K, int stride) {
    if (in < K) return 0;
    int out = (in - K + stride - 1) / stride + 1;
    if ((out - 1) * stride >= in) --out;
    return out;
}

// the window of output o along one axis: [lo, hi)
VPK_CT_FN void pool_window(int o, int K, int stride, int in, int& lo, int& hi) {
    lo = o * stride;
    hi = lo + K < in ? lo + K : in;
}

// the outputs whose window contains input i along one axis: [lo, hi] (empty when lo > hi)
VPK_CT_FN void pool_windows_of(int i, int K, int stride, int out, int& lo, int& hi) {
    const int t = i - K + 1;                                     // o stride >= t
    lo = t <= 0 ? 0 : (t + stride - 1) / stride;
    hi = i / stride;
    if (hi > out - 1) hi = out - 1;
}

// the first element in row-major scan order that is strictly greater than all before it: its flat index h W + w
VPK_CT_FN int pool_argmax(const float* plane, int W, int h0, int h1, int w0, int w1) {
    int best = h0 * W + w0;
    float m = plane[best];
    for (int h = h0; h < h1; ++h)
        for (int w = w0; w < w1; ++w) {
            const float v = plane[h * W + w];
            if (v > m) {
                m = v;
                best = h * W + w;
            }
        }
    return best;
}

// ---- LRN across channels ------------------------------------------------------------------------------------------------
// The numbers every element shares, formed once in float32: alpha / n and 2 alpha beta / n.
VPK_CT_FN float lrn_alpha_over_n(float alpha, int n) { return alpha / (float)n; }
VPK_CT_FN float lrn_back_coef(float alpha, float beta, int n) { return 2.0f * alpha * beta / (float)n; }

// s_c = k + (alpha / n) sum x_j^2 over the existing channels of the window, in rising j.  x: the channel column of one pixel,
// element j at x[j * stride].
VPK_CT_FN float lrn_scale(const float* x, int stride, int c, int C, int n, float alpha_over_n, float k) {
    const int h = n / 2, lo = c - h < 0 ? 0 : c - h, hi = c + h > C - 1 ? C - 1 : c + h;
    float sum = 0.0f;
    for (int j = lo; j <= hi; ++j) {
        const float v = x[(size_t)j * stride];
        sum += v * v;
    }
    return k + alpha_over_n * sum;
}

VPK_CT_FN float lrn_forward(float x, float s, float beta) { return x * powf(s, -beta); }

// one term of the backward's sum: dy_j y_j / s_j
VPK_CT_FN float lrn_ratio(float dy, float y, float s) { return dy * y / s; }

// dx_c = dy_c s_c^-beta - coef x_c sum_j ratio_j over the channels j whose window contains c (|j - c| <= n / 2), rising j
VPK_CT_FN float lrn_backward(const float* ratio, int stride, int c, int C, int n, float dy, float x, float s, float beta,
                             float coef) {
    const int h = n / 2, lo = c - h < 0 ? 0 : c - h, hi = c + h > C - 1 ? C - 1 : c + h;
    float sum = 0.0f;
    for (int j = lo; j <= hi; ++j) sum += ratio[(size_t)j * stride];
    return dy * powf(s, -beta) - coef * x * sum;
}

// ---- a convolution as three products ------------------------------------------------------------------------------------
struct ConvGeom {
    int C, H, W;                  // input
    int OC, K, stride, pad, groups, relu;
    int OH, OW;                   // output
    int B;                        // images of the step
#if defined(__HIPCC__)
    __host__ __device__
#endif
    int ICg() const { return C / groups; }
#if defined(__HIPCC__)
    __host__ __device__
#endif
    int OCg() const { return OC / groups; }
};

enum { GEMM_FWD = 0, GEMM_DGRAD = 1, GEMM_WGRAD = 2 };

// Per channel group g:
//   FWD    m = output channel, n = (b, oy, ox),  r = (ic, ky, kx)     Y = W X + bias, ReLU
//   DGRAD  m = input channel,  n = (b, h, w),    r = (oc, ky, kx)     dX[h] = sum dY[(h + pad - ky) / stride] W[ky], where that divides
//   WGRAD  m = output channel, n = (ic, ky, kx) and one more column for the bias,  r = (b, oy, ox)     dW = dY X^T, db = dY 1
// dY is taken through the ReLU's backward on the way in: where top <= 0 it counts as 0.
VPK_CT_FN void gemm_dims(int mode, const ConvGeom& q, int& M, int& N, int& R) {
    const int kk = q.K * q.K;
    if (mode == GEMM_FWD) { M = q.OCg(); N = q.B * q.OH * q.OW; R = q.ICg() * kk; }
    else if (mode == GEMM_DGRAD) { M = q.ICg(); N = q.B * q.H * q.W; R = q.OCg() * kk; }
    else { M = q.OCg(); N = q.ICg() * kk + 1; R = q.B * q.OH * q.OW; }
}

struct ConvPtrs {
    const float* x;               // input blob   B x C x H x W
    const float* w;               // weights      OC x ICg x K x K
    const float* bias;            // OC
    const float* top;             // output blob  B x OC x OH x OW (the ReLU's mask in the backward)
    const float* dy;              // gradient with respect to the output blob
    float* out;                   // FWD: the output blob; DGRAD: dX; WGRAD: partial[slab][OC][ICg K K + 1]
};

VPK_CT_FN float relu_back(const ConvPtrs& p, const ConvGeom& q, size_t i) {
    return (!q.relu || p.top[i] > 0.0f) ? p.dy[i] : 0.0f;
}

// x[b][g ICg + ic][oy stride - pad + ky][ox stride - pad + kx], 0 in the padding; tap = (ic, ky, kx), pix = (b, oy, ox)
VPK_CT_FN float input_at(const ConvPtrs& p, const ConvGeom& q, int g, int tap, int pix) {
    const int kk = q.K * q.K, ic = tap / kk, t = tap - ic * kk, ky = t / q.K, kx = t - ky * q.K;
    const int P = q.OH * q.OW, b = pix / P, o = pix - b * P, oy = o / q.OW, ox = o - oy * q.OW;
    const int iy = oy * q.stride - q.pad + ky, ix = ox * q.stride - q.pad + kx;
    if (iy < 0 || iy >= q.H || ix < 0 || ix >= q.W) return 0.0f;
    return p.x[(((size_t)b * q.C + g * q.ICg() + ic) * q.H + iy) * q.W + ix];
}

VPK_CT_FN float gemm_a(int mode, const ConvPtrs& p, const ConvGeom& q, int g, int m, int r) {
    const int kk = q.K * q.K;
    if (mode == GEMM_FWD) return p.w[((size_t)g * q.OCg() + m) * q.ICg() * kk + r];
    if (mode == GEMM_DGRAD) {
        const int j = r / kk, t = r - j * kk;
        return p.w[(((size_t)g * q.OCg() + j) * q.ICg() + m) * kk + t];
    }
    const int P = q.OH * q.OW, b = r / P, o = r - b * P;
    return relu_back(p, q, ((size_t)b * q.OC + g * q.OCg() + m) * P + o);
}

VPK_CT_FN float gemm_b(int mode, const ConvPtrs& p, const ConvGeom& q, int g, int r, int n) {
    const int kk = q.K * q.K;
    if (mode == GEMM_FWD) return input_at(p, q, g, r, n);
    if (mode == GEMM_WGRAD) return n == q.ICg() * kk ? 1.0f : input_at(p, q, g, n, r);
    const int j = r / kk, t = r - j * kk, ky = t / q.K, kx = t - ky * q.K;
    const int HW = q.H * q.W, b = n / HW, i = n - b * HW, h = i / q.W, w = i - h * q.W;
    const int ty = h + q.pad - ky, tx = w + q.pad - kx;
    if (ty < 0 || tx < 0) return 0.0f;
    const int oy = ty / q.stride, ox = tx / q.stride;
    if (oy * q.stride != ty || ox * q.stride != tx || oy >= q.OH || ox >= q.OW) return 0.0f;
    return relu_back(p, q, (((size_t)b * q.OC + g * q.OCg() + j) * q.OH + oy) * q.OW + ox);
}

VPK_CT_FN void gemm_store(int mode, const ConvPtrs& p, const ConvGeom& q, int g, int slab, int m, int n, float acc) {
    if (mode == GEMM_FWD) {
        const int P = q.OH * q.OW, b = n / P, o = n - b * P, oc = g * q.OCg() + m;
        float y = acc + p.bias[oc];
        if (q.relu) y = fmaxf(y, 0.0f);
        p.out[((size_t)b * q.OC + oc) * P + o] = y;
    } else if (mode == GEMM_DGRAD) {
        const int HW = q.H * q.W, b = n / HW, i = n - b * HW;
        p.out[((size_t)b * q.C + g * q.ICg() + m) * HW + i] = acc;
    } else {
        const int cols = q.ICg() * q.K * q.K + 1;
        p.out[((size_t)slab * q.OC + g * q.OCg() + m) * cols + n] = acc;
    }
}

// The weight gradient's split of its reduction (B OH OW terms) into slabs: whole chunks of `chunk` terms, as many slabs as
// bring the launch to about `target` workgroups but at least four chunks each.  A function of the geometry and B alone.
VPK_CT_FN void wgrad_slabs(const ConvGeom& q, int tile, int chunk, int target, int& slabs, int& slab_len) {
    int M, N, R;
    gemm_dims(GEMM_WGRAD, q, M, N, R);
    const int tiles = ((M + tile - 1) / tile) * ((N + tile - 1) / tile) * q.groups;
    int want = target / tiles;
    if (want < 1) want = 1;
    const int most = (R + 4 * chunk - 1) / (4 * chunk);
    if (want > most) want = most;
    slab_len = ((R + want - 1) / want + chunk - 1) / chunk * chunk;
    slabs = (R + slab_len - 1) / slab_len;
}

}  // namespace vpk_convtrain

#endif
