// lsd_host_driver.cpp -- TEST-ONLY stand-alone program over the host side of the line segment detector: detect_image
// (csrc/lsd_host.hpp) with both math policies on small images at the scales where a scaled side is 1 pixel, below 1, 1 and
// above 1, and plan_batch (csrc/lsd_plan.hpp) on a planned batch and on every refusal.  Made to be built with the host
// sanitizers and run on its own; it prints one line and returns 0 when every call answered as expected:
//     python tests/hostsim/hostbuild.py drivers
// No test runs it.
#include <stdio.h>

#include <vector>

#include "../../vanishing_points_2017_amd/csrc/lsd_host.hpp"
#include "../../vanishing_points_2017_amd/csrc/lsd_plan.hpp"

using namespace vpk_lsd;

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        ++failures;
        printf("FAILED: %s\n", what);
    }
}

// dark diagonal strokes on a light ground plus a little noise; one NaN pixel when asked for
std::vector<double> image(int w, int h, bool nan_pixel) {
    std::vector<double> img((size_t)w * h);
    unsigned s = 12345u;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            s = s * 1664525u + 1013904223u;
            const int d = (3 * x - 2 * y + 64) % 24;
            img[(size_t)y * w + x] = (d < 6 ? 40.0 : 220.0) + (double)(s >> 24) / 64.0;
        }
    if (nan_pixel) img[(size_t)(h / 2) * w + w / 2] = NAN;
    return img;
}

template <class M>
long long detect_all() {
    const int shapes[3][2] = {{8, 8}, {9, 13}, {48, 40}};
    const double scales[4] = {0.125, 0.8, 1.0, 1.25};
    long long rows = 0;
    for (const auto& sh : shapes)
        for (double scale : scales)
            for (int nan_pixel = 0; nan_pixel < 2; ++nan_pixel) {
                const std::vector<double> img = image(sh[0], sh[1], nan_pixel != 0);
                std::vector<double> out(7 * 64);
                int n = -1;
                expect(detect_image<M>(img.data(), sh[0], sh[1], scale, out.data(), 64, &n) == 0 && n >= 0, "detect_image");
                int n0 = -1;                                   // no buffer: the count alone
                expect(detect_image<M>(img.data(), sh[0], sh[1], scale, nullptr, 0, &n0) == 0 && n0 == n, "count only");
                rows += n;
            }
    const std::vector<double> img = image(8, 8, false);
    int n = 0;
    expect(detect_image<M>(img.data(), 7, 8, 0.8, nullptr, 0, &n) == -1, "a side of 7");
    expect(detect_image<M>(img.data(), 8, 8, 0.0, nullptr, 0, &n) == -1, "scale 0");
    expect(detect_image<M>(nullptr, 8, 8, 0.8, nullptr, 0, &n) == -1, "no image");
    return rows;
}

PlanRule rule_of(std::vector<int32_t> dims, std::vector<int64_t> off, double scale, size_t limit = 0) {
    const Plan p = plan_batch((int)dims.size() / 2, dims.data(), off.data(), scale, limit);
    if (p.rule == PLAN_OK) {
        expect(p.starts.size() >= 2 && p.starts.front() == 0 && p.starts.back() == (int)dims.size() / 2, "chunk starts");
        expect(p.ws_bytes >= 256 + 2048, "workspace size");
    } else {
        expect(p.image >= 0 && p.image < (int)dims.size() / 2, "the refused image");
    }
    return p.rule;
}

void plan_all() {
    const int64_t side = 1 << 20;
    expect(rule_of({8, 8, 20, 30}, {0, 64, 664}, 0.8) == PLAN_OK, "a batch of two plans");
    expect(rule_of({8, 8, 20, 30}, {0, 64, 664}, 1.0, 1) == PLAN_OK, "one image per chunk");
    expect(rule_of({8, 8, 7, 30}, {0, 64, 274}, 0.8) == PLAN_SIDE, "a side of 7");
    expect(rule_of({8, 8, 20, 30}, {0, 64, 663}, 0.8) == PLAN_OFFSETS, "offsets one short");
    expect(rule_of({8, 8, 20, 30}, {0, 64, 665}, 0.8) == PLAN_OFFSETS, "offsets one long");
    expect(rule_of({8, 8, 20, 30}, {-64, 0, 600}, 0.8) == PLAN_OFFSETS, "a negative offset");
    expect(rule_of({(int32_t)side + 1, 8}, {0, (side + 1) * 8}, 1.0) == PLAN_DIM, "width 2^20 + 1");
    expect(rule_of({(int32_t)side, 8}, {0, side * 8}, 1.25) == PLAN_DIM, "width 2^20 at scale 1.25");
    expect(rule_of({(int32_t)side, 8}, {0, side * 8}, 1.0) == PLAN_OK, "width 2^20");
    expect(rule_of({32768, 32769}, {0, (int64_t)32768 * 32769}, 1.0) == PLAN_PIXELS, "over 2^30 pixels");
    expect(rule_of({32768, 32768}, {0, (int64_t)32768 * 32768}, 1.0) == PLAN_OK, "2^30 pixels");
    expect(rule_of({7, 30}, {0, 1}, 1.0) == PLAN_SIDE, "the side before the offsets");
    expect(rule_of({(int32_t)side + 1, 8}, {0, 1}, 1.0) == PLAN_OFFSETS, "the offsets before the side limit");
    expect(rule_of({(int32_t)side, (int32_t)side}, {0, side * side}, 1.25) == PLAN_DIM, "the side limit before the pixels");
    expect(rule_of(std::vector<int32_t>(2 * 4097, 8), [] {
               std::vector<int64_t> off(4098);
               for (int b = 0; b <= 4097; ++b) off[(size_t)b] = 64 * b;
               return off;
           }(), 1.0) == PLAN_OK, "4 097 images");
}

}  // namespace

int main() {
    const long long libm = detect_all<Libm>(), portable = detect_all<Portable>();
    plan_all();
    printf("lsd_host_driver: %lld rows with libm, %lld with the portable functions, %d failures\n", libm, portable, failures);
    return failures ? 1 : 0;
}
