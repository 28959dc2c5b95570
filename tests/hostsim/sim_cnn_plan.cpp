// sim_cnn_plan.cpp -- TEST-ONLY host build of csrc/cnn_plan.hpp (plain C++, no HIP): cnn_resolve_plan as a flat int record
// for tests/test_cnn_plan.py.
#include "../../vanishing_points_2017_amd/csrc/cnn_plan.hpp"

#include <string.h>

extern "C" {

// precision_mode: vpk_cnn_set_precision's argument 0 .. 3.  out[33]:
//   0 err  1 prep_input  2 conv1  3 conv1_hands_planes  4 norm2_planes  5 norm2_hands_planes  6..8 fc6..8
//   9 + 6 i (i = 0..3: conv2..5): impl, split_tiling, chained_in, chained_out, needs_to_planes, writes_next_planes
// msg (at least 128 bytes): the error text, or empty
void sim_cnn_plan(int precision_mode, int algorithm, int fusion, int dense_presplit, int profiling, int tap, int f32_images,
                  int device_counted, int* out, char* msg) {
    CnnConfig c;
    cnn_config_set_precision(c, precision_mode);
    c.algorithm = algorithm;
    c.fusion = fusion;
    c.dense_presplit = dense_presplit;
    c.profiling = profiling != 0;
    const CnnPlan p = cnn_resolve_plan(c, tap, f32_images != 0, device_counted != 0);
    out[0] = p.err; out[1] = p.prep_input; out[2] = (int)p.conv1; out[3] = p.conv1_hands_planes;
    out[4] = p.norm2_planes; out[5] = p.norm2_hands_planes;
    for (int i = 0; i < 3; ++i) out[6 + i] = (int)p.fc[i];
    for (int i = 0; i < 4; ++i) {
        const ConvStage& s = p.conv[i];
        int* o = out + 9 + 6 * i;
        o[0] = (int)s.impl; o[1] = s.split_tiling; o[2] = s.chained_in; o[3] = s.chained_out; o[4] = s.needs_to_planes;
        o[5] = s.writes_next_planes;
    }
    strncpy(msg, p.msg ? p.msg : "", 127);
    msg[127] = 0;
}

int sim_vpk_err_state() { return VPK_ERR_STATE; }

}  // extern "C"
