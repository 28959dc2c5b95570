// cnn_calibrate.hpp -- the activation scales of the fp16-pair layers: calibration forwards on the f32 direct kernels and the
// power-of-two rule.  Included by vpk_cnn.hip after run_forward.
#ifndef VPK_CNN_CALIBRATE_HPP_
#define VPK_CNN_CALIBRATE_HPP_

namespace {

// ---- activation scales of the fp16-pair layers (cnn_conv_pieces.hpp) ----------------------------------------------------------------
// For each consuming layer (conv2..5, fc6, fc7) the largest |value| of its INPUT blob over a set of calibration rasters, computed by the
// f32 direct kernels -- which do not depend on any scale --, is brought into [32, 64) by a power of two: 2^10 of headroom up to fp16's
// 65 504 for rasters whose activations exceed the calibration set's, and an absolute error floor of 2^-25 / scale (the second piece's
// denormal spacing), i.e. below 2^-30 of the calibration maximum, for rasters whose activations are far below it.
// Built-in calibration set (vpk_cnn_load, vpk_cnn_calibrate(h, NULL, 0)), generated here with integer / single f32 operations only:
//   0  sparse noise: 15 % of the pixels 0..59 (mean 4.4: a raster of a few lines)
//   1  1000 straight strokes blended like sphere_line_plot's curves (alpha 0.1, sphere_mapping.py:62-66): mean ~48, 85 % of the
//      pixels touched, maxima ~240 -- the density of the configs[2..4] rasters (evaluation.py:12-14 with 1000 lines)
//   2  every pixel 255: the largest input the uint8 boundary admits
// The maximum over the set decides: round 5 calibrated on raster 0 alone, and dense rasters spent 3 of its 9 bits of headroom.
// Fixed for the lifetime of the loaded model unless the caller recalibrates: results never depend on earlier forwards.
constexpr int CAL_N = 6;
constexpr int CAL_LAYER[CAL_N] = {1, 2, 3, 4, 5, 6};          // conv2, conv3, conv4, conv5, fc6, fc7
constexpr int CAL_TAP[CAL_N] = {1, 3, 4, 5, 7, 8};            // taps of their inputs: pool1, pool2, conv3, conv4, pool5, fc6
constexpr int CAL_CHUNK = 8;                                   // rasters per calibration forward

// max |x| as the bit pattern of a non-negative float (ordered like unsigned integers; a NaN's pattern is above infinity's)
__global__ void absmax_kernel(const float* __restrict__ x, size_t n, unsigned* __restrict__ out) {
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned b = __builtin_bit_cast(unsigned, x[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

void builtin_calibration_rasters(std::vector<uint8_t>& img) {
    const size_t P = 500 * 500;
    img.assign(3 * P, 0);
    unsigned x = 12345u;
    auto next = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (size_t i = 0; i < P; ++i) {
        const unsigned r = next();
        img[i] = (r % 100u) < 15u ? (uint8_t)((r >> 8) % 60u) : 0;
    }
    std::vector<float> canvas(P, 0.f);
    for (int k = 0; k < 1000; ++k) {
        const int y0 = (int)(next() % 500u), y1 = (int)(next() % 500u);
        for (int c = 0; c < 500; ++c) {
            const int y = y0 + ((y1 - y0) * c) / 499;
            float& p = canvas[(size_t)y * 500 + c];
            p = p + 0.1f * (255.f - p);
        }
    }
    for (size_t i = 0; i < P; ++i) img[P + i] = (uint8_t)(canvas[i] + 0.5f);
    for (size_t i = 0; i < P; ++i) img[2 * P + i] = 255;
}

float scale_for_maximum(float m) {
    if (!(m > 0.f) || !std::isfinite(m)) return CP_DEFAULT_ASCALE;
    int ex;
    (void)std::frexp(m, &ex);                  // m = f 2^ex, f in [0.5, 1)
    ex = 6 - ex;                               // m 2^(6 - ex) in [32, 64)
    ex = ex < -100 ? -100 : (ex > 100 ? 100 : ex);
    return std::ldexp(1.f, ex);
}

// the six blob maxima over n rasters on the device
int blob_maxima(vpk_handle* h, const uint8_t* d_imgs, int n, float mx[CAL_N]) {
    vpk_cnn_state* S = h->cnn;
    DeviceBuffer<float> d_out, d_tap;
    DeviceBuffer<unsigned> d_max;
    const int chunk = n < CAL_CHUNK ? n : CAL_CHUNK;
    if (hipMalloc(d_out.out(), (size_t)chunk * OUTPUTS_PER_IMAGE * sizeof(float)) != hipSuccess ||
        hipMalloc(d_tap.out(), (size_t)chunk * A_POOL1 * sizeof(float)) != hipSuccess ||        // (the largest tapped blob)
        hipMalloc(d_max.out(), CAL_N * sizeof(unsigned)) != hipSuccess ||
        hipMemsetAsync(d_max.p, 0, CAL_N * sizeof(unsigned), h->stream) != hipSuccess)
        return vpk_fail(h, VPK_ERR_HIP, "vpk_cnn_calibrate: buffers of the calibration forwards");
    CnnConfig direct = S->cfg;                   // the f32 direct kernels: they depend on no scale
    direct.algorithm = 0; direct.fusion = 1; direct.precision = 0; direct.profiling = false;
    int rc = VPK_OK;
    for (int b0 = 0; b0 < n && rc == VPK_OK; b0 += chunk) {
        const int nb = n - b0 < chunk ? n - b0 : chunk;
        for (int i = 0; i < CAL_N && rc == VPK_OK; ++i) {
            rc = run_forward(h, direct, Images{d_imgs + (size_t)b0 * IMAGE_PIXELS, false}, nb, d_out.p, CAL_TAP[i], d_tap.p, FwdCtl{S->range_word.p, nullptr, nullptr});
            if (rc == VPK_OK) hipLaunchKernelGGL(absmax_kernel, dim3(256), dim3(256), 0, h->stream, (const float*)d_tap.p, (size_t)nb * TAP_FLOATS[CAL_TAP[i]], d_max.p + i);
        }
    }
    unsigned bits[CAL_N] = {};
    if (rc == VPK_OK && (hipStreamSynchronize(h->stream) != hipSuccess ||
                         hipMemcpy(bits, d_max.p, sizeof(bits), hipMemcpyDeviceToHost) != hipSuccess))
        rc = vpk_fail(h, VPK_ERR_HIP, "vpk_cnn_calibrate: calibration forward failed");
    for (int i = 0; i < CAL_N; ++i) memcpy(&mx[i], &bits[i], 4);
    return rc;
}

// rasters == nullptr: the built-in set
int calibrate(vpk_handle* h, const uint8_t* rasters, int n) {
    vpk_cnn_state* S = h->cnn;
    DeviceBuffer<uint8_t> d_img;
    if (!rasters) {
        std::vector<uint8_t> img;
        builtin_calibration_rasters(img);
        n = (int)(img.size() / IMAGE_PIXELS);
        if (hipMalloc(d_img.out(), img.size()) != hipSuccess ||
            hipMemcpy(d_img.p, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess)
            return vpk_fail(h, VPK_ERR_HIP, "vpk_cnn_calibrate: the built-in calibration rasters");
        rasters = d_img.p;
    }
    float mx[CAL_N];
    const int rc = blob_maxima(h, rasters, n, mx);
    d_img.reset();
    if (rc != VPK_OK) return rc;
    for (int i = 0; i < CAL_N; ++i)
        if (!std::isfinite(mx[i]))
            return vpk_fail(h, VPK_ERR_RANGE, "vpk_cnn_calibrate: a blob of the calibration forward is not finite (weights?)");
    for (int i = 0; i < CAL_N; ++i) S->L[CAL_LAYER[i]].ascale = scale_for_maximum(mx[i]);
    return VPK_OK;
}

}  // namespace
#endif
