// sim_convtrain.cpp -- TEST-ONLY host build of the per-element rules of the conv stack's training step
// (csrc/convtrain_device.hpp): shape rules, pooling windows and argmax, the LRN of one channel column, and the three index
// maps of a convolution, driven here by plain loops where vpk_convtrain.hip drives them by tiles.  For tests/test_convtrain.py.
#include "../../vanishing_points_2017_amd/csrc/convtrain_device.hpp"

namespace ct = vpk_convtrain;

extern "C" {

int sim_ct_conv_out_size(int in, int K, int stride, int pad) { return ct::conv_out_size(in, K, stride, pad); }
int sim_ct_pool_out_size(int in, int K, int stride) { return ct::pool_out_size(in, K, stride); }
void sim_ct_pool_window(int o, int K, int stride, int in, int* lo, int* hi) { ct::pool_window(o, K, stride, in, *lo, *hi); }
void sim_ct_pool_windows_of(int i, int K, int stride, int out, int* lo, int* hi) { ct::pool_windows_of(i, K, stride, out, *lo, *hi); }

// MAX pooling of `planes` planes, forward (y, idx) and backward (dx from dy and idx), thread for thread as the kernels do
void sim_ct_pool_forward(const float* x, int planes, int H, int W, int K, int stride, float* y, int32_t* idx) {
    const int OH = ct::pool_out_size(H, K, stride), OW = ct::pool_out_size(W, K, stride);
    for (int p = 0; p < planes; ++p)
        for (int oh = 0; oh < OH; ++oh)
            for (int ow = 0; ow < OW; ++ow) {
                int h0, h1, w0, w1;
                ct::pool_window(oh, K, stride, H, h0, h1);
                ct::pool_window(ow, K, stride, W, w0, w1);
                const float* src = x + (size_t)p * H * W;
                const int best = ct::pool_argmax(src, W, h0, h1, w0, w1);
                idx[((size_t)p * OH + oh) * OW + ow] = best;
                y[((size_t)p * OH + oh) * OW + ow] = src[best];
            }
}

void sim_ct_pool_backward(const float* dy, const int32_t* idx, int planes, int H, int W, int K, int stride, float* dx) {
    const int OH = ct::pool_out_size(H, K, stride), OW = ct::pool_out_size(W, K, stride);
    for (int p = 0; p < planes; ++p)
        for (int h = 0; h < H; ++h)
            for (int w = 0; w < W; ++w) {
                int oh0, oh1, ow0, ow1;
                ct::pool_windows_of(h, K, stride, OH, oh0, oh1);
                ct::pool_windows_of(w, K, stride, OW, ow0, ow1);
                float s = 0.f;
                for (int oh = oh0; oh <= oh1; ++oh)
                    for (int ow = ow0; ow <= ow1; ++ow) {
                        const size_t o = ((size_t)p * OH + oh) * OW + ow;
                        if (idx[o] == h * W + w) s += dy[o];
                    }
                dx[((size_t)p * H + h) * W + w] = s;
            }
}

// the LRN of one channel column of C values: s and y; and its backward from (x, y, s, dy)
void sim_ct_lrn_forward(const float* x, int C, int n, float alpha, float beta, float k, float* s, float* y) {
    const float aon = ct::lrn_alpha_over_n(alpha, n);
    for (int c = 0; c < C; ++c) {
        s[c] = ct::lrn_scale(x, 1, c, C, n, aon, k);
        y[c] = ct::lrn_forward(x[c], s[c], beta);
    }
}

void sim_ct_lrn_backward(const float* x, const float* y, const float* s, const float* dy, int C, int n, float alpha, float beta,
                         float* ratio, float* dx) {
    const float coef = ct::lrn_back_coef(alpha, beta, n);
    for (int c = 0; c < C; ++c) ratio[c] = ct::lrn_ratio(dy[c], y[c], s[c]);
    for (int c = 0; c < C; ++c) dx[c] = ct::lrn_backward(ratio, 1, c, C, n, dy[c], x[c], s[c], beta, coef);
}

void sim_ct_wgrad_slabs(const int32_t* geom, int tile, int chunk, int target, int* slabs, int* slab_len) {
    ct::ConvGeom q = {geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], geom[6], geom[7], geom[8], geom[9], geom[10], geom[11]};
    ct::wgrad_slabs(q, tile, chunk, target, *slabs, *slab_len);
}

// One of the three products through gemm_a / gemm_b / gemm_store, every slab summed on its own in rising r.
// geom: C, H, W, OC, K, stride, pad, groups, relu, OH, OW, B.  out: as ConvPtrs::out for the mode.
void sim_ct_gemm(int mode, const int32_t* geom, const float* x, const float* w, const float* bias, const float* top,
                 const float* dy, float* out, int slabs, int slab_len) {
    ct::ConvGeom q = {geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], geom[6], geom[7], geom[8], geom[9], geom[10], geom[11]};
    ct::ConvPtrs p = {x, w, bias, top, dy, out};
    int M, N, R;
    ct::gemm_dims(mode, q, M, N, R);
    for (int g = 0; g < q.groups; ++g)
        for (int slab = 0; slab < slabs; ++slab) {
            const int r0 = slab * slab_len, r1 = r0 + slab_len < R ? r0 + slab_len : R;
            for (int m = 0; m < M; ++m)
                for (int n = 0; n < N; ++n) {
                    float acc = 0.f;
                    for (int r = r0; r < r1; ++r) acc = fmaf(ct::gemm_a(mode, p, q, g, m, r), ct::gemm_b(mode, p, q, g, r, n), acc);
                    ct::gemm_store(mode, p, q, g, slab, m, n, acc);
                }
        }
}

}  // extern "C"
