// vpk_lsd.cpp -- line segment detector of the front end on the host (C-ABI entry vpk_lsd_detect).
//
// replaces: lsdpython.lsd.detect_line_segments(image) as called from detect_lsd_lines (evaluation.py:227-251).
// The detector itself is lsd_device.hpp, the source the GPU batch (vpk_lsd_gpu.hip) compiles too; lsd_host.hpp runs it
// for one image, serially, on the C library's libm.  lsd_device.hpp says what is restated and from where.  The detector is
// sequential by construction (region growing follows the gradient order); it is not on the hot path of any BASELINE
// config (all of them take LSD lines as given).  tests/test_frontend.py checks the contract the paper states:
// synthetic segments are recovered to sub-pixel accuracy and white noise yields (almost) no detection.
#include "../../include/vpk.h"
#include "lsd_host.hpp"

extern "C" int vpk_lsd_detect(const double* image, int width, int height, double scale, double* out, int max_segments,
                              int* n_out) {
    // a null image or count, a side below 8, a negative capacity, rows without a buffer, a scale that is not positive
    return vpk_lsd::detect_image<vpk_lsd::Libm>(image, width, height, scale, out, max_segments, n_out) ? VPK_ERR_ARG : VPK_OK;
}
