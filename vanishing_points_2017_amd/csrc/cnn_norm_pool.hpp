// cnn_norm_pool.hpp -- the f32 element-wise stages between the GEMMs: conv1's input pre-pass (prep_input_kernel), LRN + max
// pool fused (norm1 / pool1 tiled, norm2 / pool2 as a stream over the channels), pool5, and the tap-only unpad of bordered
// planes.  Included by vpk_cnn.hip (the C1_* constants: cnn_model.hpp).
#ifndef VPK_CNN_NORM_POOL_HPP_
#define VPK_CNN_NORM_POOL_HPP_

#include "cnn_prims.hpp"   // f32x4

namespace {

// conv1 input for the unfused / tapped paths (the default conv1_direct_kernel converts in its patch loader):
// float(uint8 raster) - mean (evaluation.py:35), written as the 16 stride-4 phase planes (Px = float: float image - mean)
//   P[py][px][Y][X] = x[4Y + py][4X + px]   (125 x 125 each)
// so that conv1 (11 x 11, stride 4) is a stride-1 gather for the DMA kernel: tap (kh, kw) of output (oh, ow)
// is P[kh % 4][kw % 4][oh + kh / 4][ow + kw / 4], and the 64 lanes of a gather (consecutive ow) read 256
// contiguous bytes instead of 64 words 16 bytes apart (8-16 cache lines per gather).  Measured (r1): conv1
// 2.76 -> 2.57 ms at B = 512, unchanged at B = 102.  With its MFMAs and stores removed conv1 still takes
// 0.36 of its 0.58 ms: with only 8 K-stages per tile it is bound by the issue rate of the 4-byte gather DMAs
// (about one per 40-60 cycles per CU), which a wider (16-byte, row-tiled) loader would relieve.
template <typename Px>
__global__ void prep_input_kernel(const Px* __restrict__ sphere, const float* __restrict__ mean,
                                  float* __restrict__ out, int plane) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;       // pixel within the image
    if (p >= plane) return;
    const size_t img = (size_t)blockIdx.y * plane;             // blockIdx.y = image
    const int y = p / 500, x = p - y * 500;
    const int q = ((y % C1_PH) * C1_PH + (x % C1_PH)) * (C1_PW * C1_PW) + (y / C1_PH) * C1_PW + x / C1_PH;
    out[img + q] = (float)sphere[img + p] - mean[p];
}

// Fused LRN (across channels, local_size 5, x * (1 + alpha/n * sum x^2)^-beta) + MAX pool 3x3 stride 2, ceil
// mode with clipped windows (deploy.prototxt:34-55, 82-103): the normalised map (0.6 GB at B = 102 for
// norm1) is never written to or re-read from HBM.
// (LRN_CCH, cnn_model.hpp: channels per workgroup, plus a 2-channel halo on each side)
// A workgroup owns TPH x TPW pooled outputs of 16 channels.
//   1. the raw input patch ((2 TPH + 1) x (2 TPW + 1) pixels, 16 + 4 halo channels) goes to LDS;
//   2. one thread per pixel walks the channels with a 5-deep register window and overwrites the patch in
//      place with the normalised values -- every pixel is normalised ONCE (a thread per pooled output
//      normalises each of its 9 taps itself: 2.25x the work and 9 dependent global loads per channel);
//   3. 3x3 / stride 2 max over the patch in LDS (window clipped at the border like Caffe), written into the
//      next convolution's bordered planes.
// norm2 + pool2 as a STREAM over the channels (r3).  The tiled kernel below gives a workgroup 16 channels of a small
// spatial patch: 20 / 16 of the channels and 13 x 31 / (12 x 30) of the pixels are read, in 124-byte row pieces, and it
// ran at 0.28 of the HBM rate.  Here a workgroup owns TPH pooled rows x the WHOLE width of one image -- in an unpadded
// NCHW plane that is one contiguous run of (2 TPH + 1) W floats per channel -- and walks a range of C / cgroups channels
// (plus two raw channels either side to start and end the window): a thread keeps
// the 5-deep raw window of its (up to four) pixels in registers, so every raw value is read exactly once, fully
// coalesced, CB channels (32 loads per thread) in flight; the normalised planes of a batch go to LDS (double buffered:
// one barrier per batch), the 3 x 3 / 2 maxima come out of LDS with Caffe's clipped windows and are written with the next
// convolution's border.  Same expressions in the same order as the tiled kernel: the same bits.
template <int TPH, int CB>
__global__ __launch_bounds__(256) void lrn5_pool3s2_stream_kernel(const float* __restrict__ in, float* __restrict__ out, int C,
                                                                  int H, int W, int PH, int PW, float alpha, float beta,
                                                                  int PHp, int PWp, int opad, int cgroups, const int* __restrict__ live) {
    constexpr int TR = 2 * TPH + 1, SLOTS = 4, PMAX = 256 * SLOTS;
    __shared__ float plane[2][CB][PMAX];
    const int tiles_h = (PH + TPH - 1) / TPH;
    const int th = blockIdx.x % tiles_h, cgi = (blockIdx.x / tiles_h) % cgroups, b = blockIdx.x / (tiles_h * cgroups);
    if (live && b >= *live) return;                      // (recompute pass: slots beyond the device count)
    const int cper = C / cgroups, c_lo = cgi * cper, c_hi = c_lo + cper;      // this workgroup's channels [c_lo, c_hi)
    const int ph0 = th * TPH, h0 = 2 * ph0;
    const int HW = H * W, npix = TR * W;                 // npix <= PMAX (checked by the host)
    const float* x = in + (size_t)b * C * HW + (size_t)h0 * W;
    bool ok[SLOTS];
    int off[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        off[i] = threadIdx.x + 256 * i;
        ok[i] = off[i] < npix && h0 + off[i] / W < H;    // (rows past the blob are zeros: they only meet clipped windows)
    }
    int ld_off[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) ld_off[i] = ok[i] ? off[i] : 0;
    float v0[SLOTS], v1[SLOTS], v2[SLOTS], v3[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {                    // raw values of the channels c_lo - 2 .. c_lo + 1 (zeros outside the blob)
        v0[i] = (ok[i] && c_lo >= 2) ? x[(size_t)(c_lo - 2) * HW + off[i]] : 0.f;
        v1[i] = (ok[i] && c_lo >= 1) ? x[(size_t)(c_lo - 1) * HW + off[i]] : 0.f;
        v2[i] = ok[i] ? x[(size_t)c_lo * HW + off[i]] : 0.f;
        v3[i] = (ok[i] && c_lo + 1 < C) ? x[(size_t)(c_lo + 1) * HW + off[i]] : 0.f;
    }
    const float an = alpha / 5.f;
    int buf = 0;
    float nx[CB][SLOTS], nn[CB][SLOTS];                  // raw values of this batch's / the next batch's channels (+2)
    auto fetch = [&](int cb, float (&dst)[CB][SLOTS]) {
#pragma unroll
        for (int k = 0; k < CB; ++k)
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) {            // unconditional loads (clamped addresses) first, all of them in flight ...
                const int c4 = cb + k + 2;
                dst[k][i] = x[(size_t)(c4 < C ? c4 : C - 1) * HW + ld_off[i]];
            }
    };
    auto mask = [&](int cb, float (&dst)[CB][SLOTS]) {    // ... zeroed where there is no such pixel / channel when they are used
#pragma unroll
        for (int k = 0; k < CB; ++k)
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) dst[k][i] = (ok[i] && cb + k + 2 < C) ? dst[k][i] : 0.f;
    };
    fetch(c_lo, nx);
    for (int cb = c_lo; cb < c_hi; cb += CB) {
        fetch(cb + CB, nn);                              // the next batch's loads are in flight under this batch's work
        mask(cb, nx);
#pragma unroll
        for (int k = 0; k < CB; ++k)
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) {
                const float v4 = nx[k][i];
                const float sc = 1.f + an * (v0[i] * v0[i] + v1[i] * v1[i] + v2[i] * v2[i] + v3[i] * v3[i] + v4 * v4);
                float pw_;
                if (beta == 0.75f) {
                    const float r = __builtin_amdgcn_rsqf(sc);
                    pw_ = r * __builtin_amdgcn_sqrtf(r);
                }
                else pw_ = powf(sc, -beta);
                if (off[i] < PMAX) plane[buf][k][off[i]] = v2[i] * pw_;
                v0[i] = v1[i]; v1[i] = v2[i]; v2[i] = v3[i]; v3[i] = v4;
            }
#pragma unroll
        for (int k = 0; k < CB; ++k)
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) nx[k][i] = nn[k][i];
        __syncthreads();
        for (int e = threadIdx.x; e < CB * TPH * PW; e += 256) {
            const int k = e / (TPH * PW), o = e - k * (TPH * PW);
            const int oy = o / PW, ox = o - oy * PW;
            const int ph = ph0 + oy, c = cb + k;
            if (ph >= PH || c >= c_hi) continue;
            float m = -3.402823466e38f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int r = 2 * oy + dy, q = 2 * ox + dx;
                    if (h0 + r < H && q < W) {            // Caffe clips the window at the border
                        const float v = plane[buf][k][r * W + q];
                        m = v > m ? v : m;
                    }
                }
            out[((size_t)b * C + c) * PHp * PWp + (size_t)(ph + opad) * PWp + ox + opad] = m;
        }
        buf ^= 1;
    }
}

template <int TPH, int TPW>
__global__ __launch_bounds__(256) void lrn5_pool3s2_tiled_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                 int C, int H, int W, int PH, int PW, float alpha,
                                                                 float beta, int PHp, int PWp, int opad) {
    constexpr int CC = LRN_CCH, NPL = CC + 4;
    constexpr int TR = 2 * TPH + 1, TC = 2 * TPW + 1, NPIX = TR * TC;
    __shared__ float patch[NPL][NPIX];
    const int tiles_w = (PW + TPW - 1) / TPW, tiles_h = (PH + TPH - 1) / TPH;
    const int nch = (C + CC - 1) / CC;
    int bid = blockIdx.x;
    const int tw = bid % tiles_w; bid /= tiles_w;
    const int th = bid % tiles_h; bid /= tiles_h;
    const int ch = bid % nch;
    const int b = bid / nch;
    const int c0 = ch * CC;
    const int ph0 = th * TPH, pw0 = tw * TPW;
    const int h0 = 2 * ph0, w0 = 2 * pw0;
    const int HW = H * W;
    const float* x = in + (size_t)b * C * HW;
    // 1. raw patch (zeros outside the blob: they only ever meet clipped windows or the LRN's zero padding)
    constexpr int LU = 8;                               // loads in flight per thread (the loop is latency-bound without them)
    for (int e0 = threadIdx.x; e0 < NPL * NPIX; e0 += 256 * LU) {
        float v[LU];
#pragma unroll
        for (int u = 0; u < LU; ++u) {
            const int e = e0 + u * 256;
            const int pl = e / NPIX, p = e - pl * NPIX;
            const int r = p / TC, q = p - r * TC;
            const int c = c0 - 2 + pl, h = h0 + r, w = w0 + q;
            v[u] = 0.f;
            if (e < NPL * NPIX && c >= 0 && c < C && h < H && w < W) v[u] = x[(size_t)c * HW + (size_t)h * W + w];
        }
#pragma unroll
        for (int u = 0; u < LU; ++u) {
            const int e = e0 + u * 256;
            if (e < NPL * NPIX) patch[0][e] = v[u];     // patch is contiguous: [pl][p] == flat e
        }
    }
    __syncthreads();
    // 2. normalise in place, one thread per pixel
    const float an = alpha / 5.f;
    for (int p = threadIdx.x; p < NPIX; p += 256) {
        float v0 = patch[0][p], v1 = patch[1][p], v2 = patch[2][p], v3 = patch[3][p];
#pragma unroll
        for (int k = 0; k < CC; ++k) {
            const float v4 = patch[k + 4][p];
            const float sc = 1.f + an * (v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3 + v4 * v4);
            float pw_;
            if (beta == 0.75f) {                         // v_rsq_f32 / v_sqrt_f32 (1 ulp, sc >= 1); the IEEE-exact library
                const float r = __builtin_amdgcn_rsqf(sc);   // forms expand to ~25 VALU instructions each
                pw_ = r * __builtin_amdgcn_sqrtf(r);
            }
            else pw_ = powf(sc, -beta);
            patch[k + 2][p] = v2 * pw_;                  // plane k+2 holds channel c0+k; its raw value lives in v2
            v0 = v1; v1 = v2; v2 = v3; v3 = v4;
        }
    }
    __syncthreads();
    // 3. pool
    for (int e = threadIdx.x; e < CC * TPH * TPW; e += 256) {
        const int k = e / (TPH * TPW), o = e - k * (TPH * TPW);
        const int oy = o / TPW, ox = o - oy * TPW;
        const int ph = ph0 + oy, pw = pw0 + ox, c = c0 + k;
        if (ph >= PH || pw >= PW || c >= C) continue;
        float m = -3.402823466e38f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int r = 2 * oy + dy, q = 2 * ox + dx;
                if (h0 + r < H && w0 + q < W) {          // Caffe clips the window at the border
                    const float v = patch[k + 2][r * TC + q];
                    m = v > m ? v : m;
                }
            }
        out[((size_t)b * C + c) * PHp * PWp + (size_t)(ph + opad) * PWp + pw + opad] = m;
    }
}

// pool5 (deploy.prototxt:181-191): 3 x 3 / 2 max pool of unpadded 30 x 30 planes -> 15 x 15 (ceil mode: the last window is
// clipped).  A workgroup stages PL whole planes in LDS with 16-byte loads (a plane is 3600 contiguous bytes; the windows
// of neighbouring outputs overlap, and one thread per output reading its nine values from HBM ran at 2.3 TB/s), then
// every thread takes pooled outputs out of LDS; stores are contiguous.  Maxima: order-free, same values.
template <int PL>
__global__ __launch_bounds__(256) void pool5_kernel(const float* __restrict__ in, float* __restrict__ out, long long planes,
                                                    const int* __restrict__ live) {
    constexpr int H = 30, W = 30, P = 15, HW = H * W, PP = P * P;
    __shared__ __attribute__((aligned(16))) float s[PL * HW];
    const long long p0 = (long long)blockIdx.x * PL;
    if (live && p0 >= (long long)*live * 256) return;    // (recompute pass: the 256 planes of each image beyond the device count)
    const int np = planes - p0 < PL ? (int)(planes - p0) : PL;
    const f32x4* src = reinterpret_cast<const f32x4*>(in + p0 * HW);
    for (int q = threadIdx.x; q < np * HW / 4; q += 256) reinterpret_cast<f32x4*>(s)[q] = src[q];
    __syncthreads();
    float* dst = out + p0 * PP;
    for (int e = threadIdx.x; e < np * PP; e += 256) {
        const int pl = e / PP, o = e - pl * PP;
        const int py = o / P, px = o - py * P;
        const float* x = s + pl * HW + (2 * py) * W + 2 * px;
        const bool by = 2 * py + 2 < H, bx = 2 * px + 2 < W;     // (only the last row / column of windows is clipped)
        float m = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[W], x[W + 1]));
        if (bx) m = fmaxf(m, fmaxf(x[2], x[W + 2]));
        if (by) m = fmaxf(m, fmaxf(x[2 * W], x[2 * W + 1]));
        if (bx && by) m = fmaxf(m, x[2 * W + 2]);
        dst[e] = m;
    }
}

// interior of bordered planes -> dense (taps only)
__global__ void unpad_kernel(const float* __restrict__ in, float* __restrict__ out, long long planes, int H, int W,
                             int Hp, int Wp, int pad) {
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= planes * H * W) return;
    const int w = (int)(idx % W), hh = (int)((idx / W) % H);
    const long long pl = idx / ((long long)W * H);
    out[idx] = in[((size_t)pl * Hp + hh + pad) * Wp + w + pad];
}

}  // namespace
#endif
