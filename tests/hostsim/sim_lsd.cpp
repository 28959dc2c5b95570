// sim_lsd.cpp -- TEST-ONLY g++ build of the host line segment detector (csrc/lsd_host.hpp over csrc/lsd_device.hpp, both
// unmodified).  sim_lsd runs it on glibc's libm: tests/test_hostsim_lsd.py holds the product's clang build, vpk_lsd_detect,
// to it bit for bit.  sim_lsd_portable runs it with the portable math policy (lsd_portable_math.hpp): the rows recorded in
// tests/golden/lsd/lsd_portable.npz, and the rows the GPU must reproduce byte for byte under vpk_lsd_set_math(h, 1)
// (tests/test_gpu_lsd_exact.py).  It is not a product path: nothing in the package builds, loads or links it.
#include "../../vanishing_points_2017_amd/csrc/lsd_host.hpp"

using namespace vpk_lsd;

extern "C" int sim_lsd(const double* image, int width, int height, double scale, double* out, int max_segments, int* n_out) {
    return detect_image<Libm>(image, width, height, scale, out, max_segments, n_out);
}

extern "C" int sim_lsd_portable(const double* image, int width, int height, double scale, double* out, int max_segments,
                                int* n_out) {
    return detect_image<Portable>(image, width, height, scale, out, max_segments, n_out);
}
