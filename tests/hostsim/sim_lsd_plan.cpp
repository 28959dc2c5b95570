// sim_lsd_plan.cpp -- TEST-ONLY host build of csrc/lsd_plan.hpp: what vpk_lsd_detect_batch decides before it launches --
// the rules, every image's workspace offsets, the chunks -- callable from the CPU tests (tests/test_lsd_plan.py).  The
// header is plain C++, so this needs no hip_sim.hpp.
#include "../../vanishing_points_2017_amd/csrc/lsd_plan.hpp"

using namespace vpk_lsd;

extern "C" {

// returns the rule (PlanRule) and *image, the image that failed it.  When the batch plans: offsets[7 b ..]: aux, scaled, ang,
// grad, order, reg, used of image b; geom[2 b ..]: xs, ys; starts: the chunk starts and the batch (at most starts_cap of
// *n_starts are written); *ws_bytes, *max_c.
int sim_lsd_plan(int batch, const int32_t* dims, const int64_t* pix_offsets, double scale, unsigned long long limit, int* image,
                 long long* offsets, int* geom, int* starts, int starts_cap, int* n_starts, unsigned long long* ws_bytes,
                 int* max_c) {
    const Plan p = plan_batch(batch, dims, pix_offsets, scale, (size_t)limit);
    *image = p.image;
    if (p.rule) return p.rule;
    for (int b = 0; b < batch; ++b) {
        const ImgDesc& d = p.desc[(size_t)b];
        const long long o[7] = {d.aux, d.scaled, d.ang, d.grad, d.order, d.reg, d.used};
        for (int k = 0; k < 7; ++k) offsets[7 * b + k] = o[k];
        geom[2 * b] = d.xs;
        geom[2 * b + 1] = d.ys;
        if (d.b != b || d.in_off != pix_offsets[b] || d.w != dims[2 * b] || d.h != dims[2 * b + 1]) return -1;
    }
    *n_starts = (int)p.starts.size();
    for (int c = 0; c < *n_starts && c < starts_cap; ++c) starts[c] = p.starts[(size_t)c];
    *ws_bytes = p.ws_bytes;
    *max_c = p.max_c;
    return PLAN_OK;
}

int sim_lsd_plan_code(int rule) { return plan_code((PlanRule)rule); }

int sim_lsd_plan_meta_bytes() { return (int)sizeof(Meta); }

}  // extern "C"
