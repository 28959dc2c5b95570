// sim_detect.cpp -- TEST-ONLY host build of the detector glue's arithmetic (csrc/detect_device.hpp, unmodified): the rank of
// a VP under the order rule and the conversion to pixels are the product's code, run serially; only the loops over images,
// VPs and rows that the kernels of vpk_detect.hip spread over lanes are written out here.  tests/test_detector.py checks it
// against NumPy; tests/test_gpu_detector.py checks the GPU against it byte for byte.
// It is not a product path: nothing in the package builds, loads or links it.
#include "../../vanishing_points_2017_amd/csrc/detect_device.hpp"

using namespace vpk_det;

extern "C" {

// counts batch x max_vp, num_vp batch -> order batch x maxbest (vpk_vp_order_batch)
int sim_vp_order(int batch, int max_vp, const double* counts, const int32_t* num_vp, int maxbest, int32_t* order) {
    if (batch < 0 || max_vp < 1 || max_vp > MAX_VP || maxbest < 1 || maxbest > MAX_VP) return -1;
    for (long long b = 0; b < batch; ++b) {
        const int M = clamp_num_vp(num_vp[b], max_vp);
        const int nb = M < maxbest ? M : maxbest;
        const double* c = counts + b * max_vp;
        int32_t* o = order + b * maxbest;
        for (int q = nb; q < maxbest; ++q) o[q] = 0;
        for (int i = 0; i < M; ++i) {
            const int rank = vp_rank(c, M, i);
            if (rank < maxbest) o[rank] = i;
        }
    }
    return 0;
}

// vpk_to_pixels_batch; each output may be NULL
int sim_to_pixels(int batch, const int32_t* dims, const int64_t* line_offsets, const double* lp, int max_vp, const double* vp,
                  const int32_t* num_vp, const double* horizon, double* lp_px, double* vp_px, double* horizon_px) {
    for (long long b = 0; b < batch; ++b) {
        const int w = dims[2 * b], h = dims[2 * b + 1];
        if (lp_px)
            for (long long r = line_offsets[b]; r < line_offsets[b + 1]; ++r) segment_to_px(lp + 4 * r, w, h, lp_px + 4 * r);
        if (vp_px) {
            const int M = clamp_num_vp(num_vp[b], max_vp);
            for (int k = 0; k < max_vp; ++k) {
                double* o = vp_px + (b * max_vp + k) * 2;
                if (k < M) vp_to_px(vp + (b * max_vp + k) * 3, w, h, o);
                else o[0] = o[1] = quiet_nan();
            }
        }
        if (horizon_px)
            for (int e = 0; e < 2; ++e) {
                const double* p = horizon + b * 15 + 3 * e;
                point_to_px(p[0], p[1], w, h, horizon_px + (b * 2 + e) * 2);
            }
    }
    return 0;
}

}  // extern "C"
