// sim_frontend.cpp -- TEST-ONLY host build of the GPU image front end's arithmetic (csrc/image_device.hpp, unmodified): the
// Lanczos weights, both integer resize passes, the grey levels and the rows -> lines step are the product's code, run
// serially; only the orchestration around them -- grid-wide launches over a batch, the deduplicated weight tables of
// vpk_frontend.hip -- is a loop here.  tests/test_hostsim_frontend.py checks it against Pillow and numpy;
// tests/test_gpu_frontend_device.py checks the GPU against it byte for byte.
// It is not a product path: nothing in the package builds, loads or links it.
#include "../../vanishing_points_2017_amd/csrc/image_device.hpp"

#include <vector>

using namespace vpk_img;

namespace {

struct Axis {
    int ksize = 0;                 // 0: the pass is skipped
    std::vector<int32_t> bounds, coeffs;
    Axis(int in, int out) {
        if (in == out) return;
        ksize = lanczos_ksize(in, out);
        bounds.resize(2 * (size_t)out);
        coeffs.resize((size_t)out * ksize);
        std::vector<double> scratch((size_t)ksize);
        lanczos_coeffs(in, out, ksize, bounds.data(), coeffs.data(), scratch.data());
    }
};

}  // namespace

extern "C" {

// one image: in_w x in_h x ch uint8 -> resized out_w x out_h x ch uint8 (may be NULL) and grey out_w x out_h fp64
int sim_prepare(const uint8_t* in, int in_w, int in_h, int ch, int out_w, int out_h, uint8_t* resized, double* grey) {
    if (!in || !grey || (ch != 1 && ch != 3) || in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1) return -1;
    const Axis ax(in_w, out_w), ay(in_h, out_h);
    std::vector<uint8_t> tmp;
    const uint8_t* src = in;
    if (ax.ksize) {                // horizontal pass first, clipped to uint8
        tmp.resize((size_t)out_w * in_h * ch);
        for (int y = 0; y < in_h; ++y)
            for (int x = 0; x < out_w; ++x)
                for (int c = 0; c < ch; ++c)
                    tmp[((size_t)y * out_w + x) * ch + c] =
                        resample_px(in + ((long long)y * in_w + ax.bounds[2 * x]) * ch + c, ch, ax.bounds[2 * x + 1],
                                    &ax.coeffs[(size_t)x * ax.ksize]);
        src = tmp.data();
    }
    const long long row = (long long)out_w * ch;
    for (int y = 0; y < out_h; ++y)
        for (int x = 0; x < out_w; ++x) {
            const long long i = (long long)y * out_w + x;
            uint8_t px[3];
            for (int c = 0; c < ch; ++c)
                px[c] = ay.ksize ? resample_px(src + ay.bounds[2 * y] * row + (long long)x * ch + c, row, ay.bounds[2 * y + 1],
                                               &ay.coeffs[(size_t)y * ay.ksize])
                                 : src[i * ch + c];
            if (resized)
                for (int c = 0; c < ch; ++c) resized[i * ch + c] = px[c];
            grey[i] = ch == 3 ? grey_rgb(px[0], px[1], px[2]) : grey_l(px[0]);
        }
    return 0;
}

// n detector rows (7 doubles) of a w x h image -> lp (n x 4), l (n x 3)
int sim_rows_to_lines(const double* rows, int n, int w, int h, double* lp, double* l) {
    for (int i = 0; i < n; ++i) row_to_line(rows + 7 * (long long)i, w, h, lp + 4 * (long long)i, l + 3 * (long long)i);
    return 0;
}

}  // extern "C"
