// sim_emstep.cpp -- TEST-ONLY host build of csrc/emstep_device.hpp (see hip_sim.hpp): the batched weights, M-step and
// initial VPs as the library's kernel runs them, with one workgroup of one lane -- which therefore takes every image of the
// batch in turn, in ONE slot that is not cleared between them.  The slot and Shared start out as garbage.
#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/emstep_device.hpp"

using namespace vpk;

static void run(EmstepArgs& a, const std::vector<EmstepImage>& img, long long slot) {
    std::vector<double> ws((size_t)slot + EMSTEP_SPARE_DOUBLES);
    memset(ws.data(), 0xff, ws.size() * sizeof(double));
    memset(g_sim_lds, 0xff, sizeof(g_sim_lds));
    a.img = img.data();
    a.ws = ws.data();
    a.slot_doubles = slot;
    emstep_run(a);
}

extern "C" {

// returns the number of images that were processed
int sim_weight_matrix_batch(int batch, const long long* line_off, const long long* vp_off, const double* p_vl, const double* lweight,
                            const long long* lsim_off, const double* lsim, double bias, int wt_doubles, double* w_out) {
    std::vector<EmstepImage> img;
    const long long slot = emstep_plan(batch, line_off, vp_off, lsim_off, EMSTEP_WEIGHTS, 1, img);
    EmstepArgs a = {};
    a.op = EMSTEP_WEIGHTS;
    a.count = (int)img.size();
    a.wt_doubles = wt_doubles > 0 ? wt_doubles : WT_DOUBLES;
    a.p_vl = p_vl; a.lweight = lweight; a.lsim = lsim; a.bias = bias; a.w_out = w_out;
    run(a, img, slot);
    return a.count;
}

int sim_mstep_batch(int batch, const long long* line_off, const long long* vp_off, const double* l, const double* w, const double* lvsq,
                    const double* p_vl, const long long* assoc, const double* cur, double max_stdd, double s_thresh, double* vp_out,
                    double* s_out, double* err_out, int* removed_out, int* valid_out, double* max_err_out) {
    std::vector<EmstepImage> img;
    const long long slot = emstep_plan(batch, line_off, vp_off, nullptr, EMSTEP_MSTEP, 1, img);
    EmstepArgs a = {};
    a.op = EMSTEP_MSTEP;
    a.count = (int)img.size();
    a.wt_doubles = WT_DOUBLES;
    a.l = l; a.w = w; a.lvsq = lvsq; a.p_vl = p_vl; a.cur = cur; a.assoc = lvsq ? assoc : nullptr;
    a.max_stdd = max_stdd; a.s_thresh = s_thresh;
    a.vp_out = vp_out; a.s_out = s_out; a.err_out = err_out; a.max_err_out = max_err_out;
    a.removed_out = removed_out; a.valid_out = valid_out;
    run(a, img, slot);
    return a.count;
}

int sim_init_vps_batch(int batch, const float* cnn, const unsigned char* sphere, int ssize, int num_max, double* v0_out, int* m0_out,
                       float* weights_out) {
    EmstepArgs a = {};
    a.op = EMSTEP_INIT;
    a.count = batch;
    a.wt_doubles = WT_DOUBLES;
    a.cnn = cnn; a.sphere = sphere; a.ssize = ssize; a.num_max = num_max;
    a.v0_out = v0_out; a.m0_out = m0_out; a.weights_out = weights_out;
    run(a, std::vector<EmstepImage>(), 0);
    return batch;
}

}  // extern "C"
