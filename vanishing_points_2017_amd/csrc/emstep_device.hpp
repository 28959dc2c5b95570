// emstep_device.hpp -- the EM update outside the EM, batched: weight_matrix (vp_localisation.py:515-524), the M-step
// (calc_new_vanishing_point :453-479 with the variance / error / removal step around it, :284-322 soft, :353-392 hard) and
// find_initial_vps (:111-165) for many images per launch.  Every image is processed by one workgroup through the bodies of
// the single-image entry points (em_hooks.hpp: hook_weight_matrix, hook_mstep, hook_mstep_full, hook_init_vps); nothing here
// restates a phase.  What this header adds is the loop around them: a workgroup takes SEVERAL images, one after the other.
//
// Two users compile this file unmodified: vpk_emstep.hip (one kernel, `op` selects the body) and tests/hostsim/sim_emstep.cpp
// (g++ through hip_sim.hpp: one workgroup of one lane, which therefore takes every image of the batch in turn).
//
// Workspace.  The grid is min(active images, cap) workgroups and the workspace holds ONE slot per workgroup, sized for the
// largest image of the batch -- not one per image.  Workgroup q takes the images q, q + grid, ... of a largest-first order
// (emstep_plan).  Inside its slot every image lays its arrays out as the single-image entry point does for an image of its
// size (EmstepImage::L): strides and pass widths, and with them the bits, are those of the single call by construction.
//
// A second image in the same workgroup.  The hook bodies end in copy-out loops without a closing barrier (hook_get_matrix,
// the vp_out loops) and begin by filling Shared and the slot, so the loop puts a block_sync() between two images and
// resets what a body may take for fresh: sh.ibuf[2] (lsim not finite), sh.ibuf[5] (operand panel in LDS), sh.flags, sh.M.
#ifndef VPK_EMSTEP_DEVICE_HPP_
#define VPK_EMSTEP_DEVICE_HPP_

#include "em_hooks.hpp"

#include <algorithm>
#include <vector>

namespace vpk {

constexpr int EMSTEP_WEIGHTS = 0, EMSTEP_MSTEP = 1, EMSTEP_INIT = 2;
// behind every slot: what an output the caller left out is written to instead (removed: MAXM ints; weights: NCELL floats)
constexpr size_t EMSTEP_SPARE_DOUBLES = 256;
static_assert(MAXM * sizeof(int) + NCELL * sizeof(float) <= EMSTEP_SPARE_DOUBLES * sizeof(double), "spare outputs");

// one image that has lines and VPs, in launch order
struct EmstepImage {
    long long n0, m0;     // its first line and first VP
    long long mat;        // element of its [m][n] matrices
    long long lsim;       // element of its N x N lsim (weights)
    int b, N, M, pad;
    EmLayout L;           // its arrays inside the workgroup's slot
};

struct EmstepArgs {
    int op;
    int count;                       // images to process: the active ones (weights, M-step), the batch (initial VPs)
    const EmstepImage* img;          // weights, M-step: count records, largest N first
    double* ws;                      // one slot of slot_doubles per workgroup (+ EMSTEP_SPARE_DOUBLES)
    long long slot_doubles;
    int wt_doubles, smoother;
    // weights
    const double *p_vl, *lweight, *lsim;
    double bias;
    double* w_out;
    // M-step: lvsq null = positions only (hook_mstep); assoc null = soft
    const double *l, *w, *lvsq, *cur;
    const long long* assoc;
    double max_stdd, s_thresh;
    double *vp_out, *s_out, *err_out, *max_err_out;
    int *removed_out, *valid_out;
    // initial VPs
    const float* cnn;
    const unsigned char* sphere;
    int ssize, num_max;
    double* v0_out;
    int* m0_out;
    float* weights_out;
};

// The launch order of a batch and the slot it needs (host).  Image b has lines [line_off[b], line_off[b + 1]) and VPs
// [vp_off[b], vp_off[b + 1]); images without lines or without VPs get no record.  Largest N first (stable), as vpk_em_batch
// orders its queue.  The layouts are the single-image entry points': every array of the weighted EM for the weights
// (vpk_weight_matrix), the unweighted one for the M-step (vpk_mstep, vpk_mstep_full).
inline long long emstep_plan(int batch, const long long* line_off, const long long* vp_off, const long long* lsim_off, int op,
                             int nwaves, std::vector<EmstepImage>& img) {
    img.clear();
    long long mat = 0, slot = 0;
    for (int b = 0; b < batch; ++b) {
        const long long n = line_off[b + 1] - line_off[b], m = vp_off[b + 1] - vp_off[b];
        if (n > 0 && m > 0) {
            EmstepImage r = {};
            r.n0 = line_off[b]; r.m0 = vp_off[b]; r.mat = mat; r.lsim = lsim_off ? lsim_off[b] : 0;
            r.b = b; r.N = (int)n; r.M = (int)m;
            r.L = em_layout((int)n, (int)em_align((size_t)m, 8), nwaves, op == EMSTEP_WEIGHTS, false);
            slot = std::max(slot, (long long)r.L.total_doubles);
            img.push_back(r);
        }
        mat += n * m;
    }
    std::stable_sort(img.begin(), img.end(), [](const EmstepImage& x, const EmstepImage& y) { return x.N > y.N; });
    return slot;
}

// between two images of one workgroup: the previous body's copy-out has finished, and nothing of it is taken for fresh
VPK_DEV void emstep_next_image() {
    Shared& sh = SH();
    block_sync();
    if (tid() == 0) { sh.ibuf[2] = 0; sh.ibuf[5] = 0; sh.flags = 0; sh.M = 0; }
    block_sync();
}

VPK_DEV EmCtx emstep_ctx(const EmstepArgs& a, int smoother) {
    EmCtx c{};
    c.wt_doubles = a.wt_doubles; c.smoother = smoother;
    return c;
}

VPK_DEVFN void emstep_weights(const EmstepArgs& a, const EmstepImage& r, double* slot) {
    EmCtx c = emstep_ctx(a, a.smoother);
    bind_scratch(c, slot, r.L, false);
    hook_weight_matrix(c, r.N, r.M, a.p_vl + r.mat, a.lweight + r.n0, a.lsim + r.lsim, a.bias, a.w_out + r.mat);
}

VPK_DEVFN void emstep_mstep(const EmstepArgs& a, const EmstepImage& r, double* slot) {
    Shared& sh = SH();
    const int N = r.N, M = r.M;
    int* spare = (int*)(slot + a.slot_doubles);
    if (!a.lvsq) {                                            // positions only, from unit state (vpk_mstep)
        EmCtx c = emstep_ctx(a, 0);
        bind_scratch(c, slot, r.L, false);
        // hook_mstep tells a row without a new VP by its s not being NaN and does not set s itself: whatever the LDS held --
        // the previous image's variances, or another kernel's data -- must not pass for one (its barrier publishes this)
        for (int k = tid(); k < M; k += nthreads()) sh.s[k] = -1.0;
        hook_mstep(c, N, M, a.l + 3 * r.n0, a.w + r.mat, a.vp_out + 3 * r.m0, a.valid_out ? a.valid_out + r.m0 : nullptr);
        if (a.removed_out)
            for (int k = tid(); k < M; k += nthreads()) a.removed_out[r.m0 + k] = sh.removed[k];
        return;
    }
    EmCtx c = emstep_ctx(a, a.smoother);
    bind_scratch(c, slot, r.L, false);
    const int* assoc = nullptr;
    if (a.assoc) {
        // the caller's int64 association (what vpk_vp_line_counts_batch writes) into the slot's ints; an entry outside
        // [0, M) -- the -1 of an outlier -- selects no VP.  hook_mstep_full then copies c.assoc onto itself, thread for thread.
        for (int q = tid(); q < N; q += nthreads()) {
            const long long v = a.assoc[r.n0 + q];
            c.assoc[q] = (v < 0 || v >= M) ? -1 : (int)v;
        }
        assoc = (const int*)c.assoc;
    }
    hook_mstep_full(c, N, M, a.l + 3 * r.n0, a.w + r.mat, a.lvsq + r.mat, a.p_vl + r.mat, assoc, a.cur + 3 * r.m0, a.max_stdd,
                    a.s_thresh, a.vp_out + 3 * r.m0, a.s_out + r.m0, a.err_out + r.m0,
                    a.removed_out ? a.removed_out + r.m0 : spare);
    // (mstep's closing barrier has published sh.s and sh.err)  a row was written exactly where s left its -1: the M-step
    // stores exp(..) or a NaN there, never -1
    if (a.valid_out)
        for (int k = tid(); k < M; k += nthreads()) a.valid_out[r.m0 + k] = (sh.s[k] == -1.0) ? 0 : 1;
    if (a.max_err_out && tid() == 0) a.max_err_out[r.b] = max_err_of(sh, M);
}

VPK_DEVFN void emstep_init(const EmstepArgs& a, int b, double* slot) {
    Shared& sh = SH();
    EmCtx c = emstep_ctx(a, 0);
    double* v0 = a.v0_out + 3 * (size_t)a.num_max * b;
    float* spare = (float*)(slot + a.slot_doubles) + MAXM;
    hook_init_vps(c, a.cnn + (size_t)NCELL * b, a.sphere + (size_t)a.ssize * a.ssize * b, a.ssize, a.num_max, v0, a.m0_out + b,
                  a.weights_out ? a.weights_out + (size_t)NCELL * b : spare);
    for (int k = 3 * sh.M + tid(); k < 3 * a.num_max; k += nthreads()) v0[k] = 0.0;   // (sh.M: published inside initial_vps)
}

// the kernel's body: workgroup q takes the images q, q + grid, ...
VPK_DEV void emstep_run(const EmstepArgs& a) {
    double* slot = a.ws + (size_t)block_id() * (size_t)(a.slot_doubles + (long long)EMSTEP_SPARE_DOUBLES);
    bool first = true;
    for (int i = block_id(); i < a.count; i += nblocks()) {
        if (!first) emstep_next_image();
        first = false;
        if (a.op == EMSTEP_WEIGHTS) emstep_weights(a, a.img[i], slot);
        else if (a.op == EMSTEP_MSTEP) emstep_mstep(a, a.img[i], slot);
        else emstep_init(a, i, slot);
    }
}

}  // namespace vpk
#endif
