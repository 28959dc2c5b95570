// vpk_emstep.hip -- the EM update outside the EM, batched: vpk_weight_matrix_batch, vpk_mstep_batch and vpk_init_vps_batch
// (see include/vpk.h).  One kernel; `op` selects the body, which is the single-image entry point's (em_hooks.hpp) inside
// emstep_device.hpp's loop over the workgroup's images.  Compiled with -ffp-contract=off like the EM unit.
#include "emstep_device.hpp"
#include "batch_args.hpp"
#include "em_plan.hpp"
#include "vpk_internal.hpp"

using namespace vpk;

namespace {

constexpr int EMSTEP_THREADS = EM_THREADS, EMSTEP_WAVES = EM_WAVES;   // the EM workgroup's shape: the phase functions are tuned for 8 waves
constexpr long long EMSTEP_NMAX = 32768;

__global__ __launch_bounds__(EMSTEP_THREADS) void emstep_kernel(EmstepArgs a) { emstep_run(a); }

// the checks the two ragged entries share; *done = nothing to launch
int check_batch(vpk_handle* h, int batch, const int64_t* line_off, const int64_t* vp_off, const char* who, bool* done) {
    const BatchRule r = batch_pair(batch, line_off, vp_off, EMSTEP_NMAX, MAXM);
    *done = r != BATCH_OK;
    if (r == BATCH_OK || r == BATCH_EMPTY) return VPK_OK;
    return vpk_fail(h, batch_code(r), r == BATCH_VPS ? "emstep: an image has more than 64 VPs"
                                      : r == BATCH_LINES ? "emstep: an image has more than 32768 lines" : who);
}

// The grid -- min(count, cap), fewer where the slots would not fit half of the device memory --, the workspace, the records
// and the launch.  lds_bytes / a.wt_doubles: the caller's.
int launch(vpk_handle* h, EmstepArgs& a, const std::vector<EmstepImage>& img, long long slot_doubles, int per_cu, size_t lds_bytes,
           const char* who) {
    VPK_HIP(h, hipSetDevice(h->device));
    int grid = h->cu_share * per_cu;
    if (h->em_max_workgroups > 0) grid = h->em_max_workgroups;
    if (grid > a.count) grid = a.count;
    if (grid < 1) grid = 1;
    const size_t stride = ((size_t)slot_doubles + EMSTEP_SPARE_DOUBLES) * sizeof(double);
    const size_t budget = h->total_mem / 2;
    if (stride > budget) return vpk_fail(h, VPK_ERR_LIMIT, "emstep: the workspace of the largest image exceeds half of the device memory");
    while (grid > 1 && (size_t)grid * stride > budget) grid /= 2;
    if (!h->emstep_ready) {
        VPK_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(emstep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)EM_LDS_BYTES_BIG));
        h->emstep_ready = true;
    }
    int rc = vpk_reserve(h, &h->emstep_ws, &h->emstep_ws_bytes, (size_t)grid * stride, "hipMalloc(emstep workspace)");
    if (rc) return rc;
    if (!img.empty()) {
        rc = vpk_stage_upload(h, h->emstep_hdr, img.data(), img.size() * sizeof(EmstepImage), who);
        if (rc) return rc;
        a.img = (const EmstepImage*)h->emstep_hdr.dev;
    }
    a.ws = (double*)h->emstep_ws;
    a.slot_doubles = slot_doubles;
    hipLaunchKernelGGL(emstep_kernel, dim3((unsigned)grid), dim3(EMSTEP_THREADS), lds_bytes, h->stream, a);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // namespace

extern "C" {

int vpk_weight_matrix_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets, const double* p_vl,
                            const double* lweight, const int64_t* lsim_offsets, const double* lsim, double bias, double* w_out) {
    if (!h) return VPK_ERR_ARG;
    bool done;
    int rc = check_batch(h, batch, line_offsets, vp_offsets, "vpk_weight_matrix_batch: bad batch or offsets", &done);
    if (rc || done) return rc;
    if (!lsim_offsets) return vpk_fail(h, VPK_ERR_ARG, "vpk_weight_matrix_batch: null lsim_offsets");
    if (batch_slots(batch, line_offsets, lsim_offsets))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_weight_matrix_batch: lsim_offsets leave image b less than N_b^2 elements");
    std::vector<EmstepImage> img;
    const long long slot = emstep_plan(batch, (const long long*)line_offsets, (const long long*)vp_offsets,
                                       (const long long*)lsim_offsets, EMSTEP_WEIGHTS, EMSTEP_WAVES, img);
    if (img.empty()) return VPK_OK;
    if (!p_vl || !lweight || !lsim || !w_out) return vpk_fail(h, VPK_ERR_ARG, "vpk_weight_matrix_batch: null buffer");
    // the batch kernel's LDS budget (em_plan.hpp), so that an image takes the smoother it takes there and in vpk_weight_matrix
    const EmMode mode = em_mode(h->em_lds_doubles);
    EmstepArgs a = {};
    a.op = EMSTEP_WEIGHTS;
    a.count = (int)img.size();
    a.wt_doubles = mode.wt_doubles; a.smoother = h->em_smoother;
    a.p_vl = p_vl; a.lweight = lweight; a.lsim = lsim; a.bias = bias; a.w_out = w_out;
    return launch(h, a, img, slot, 1, mode.lds_bytes, "vpk_weight_matrix_batch: records");
}

int vpk_mstep_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets, const double* l,
                    const double* w, const double* lvsq, const double* p_vl, const int64_t* assoc, const double* cur,
                    double max_stdd, double s_thresh, double* vp_out, double* s_out, double* err_out, int32_t* removed_out,
                    int32_t* valid_out, double* max_err_out) {
    if (!h) return VPK_ERR_ARG;
    bool done;
    int rc = check_batch(h, batch, line_offsets, vp_offsets, "vpk_mstep_batch: bad batch or offsets", &done);
    if (rc || done) return rc;
    if ((lvsq == nullptr) != (p_vl == nullptr)) return vpk_fail(h, VPK_ERR_ARG, "vpk_mstep_batch: lvsq and p_vl are given together or not at all");
    const bool full = lvsq != nullptr;
    if (!full && (s_out || err_out || max_err_out))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_mstep_batch: s_out, err_out and max_err_out need lvsq and p_vl");
    std::vector<EmstepImage> img;
    const long long slot = emstep_plan(batch, (const long long*)line_offsets, (const long long*)vp_offsets, nullptr, EMSTEP_MSTEP,
                                       EMSTEP_WAVES, img);
    if (img.empty()) return VPK_OK;
    if (!l || !w || !vp_out || (full && (!cur || !s_out || !err_out))) return vpk_fail(h, VPK_ERR_ARG, "vpk_mstep_batch: null buffer");
    EmstepArgs a = {};
    a.op = EMSTEP_MSTEP;
    a.count = (int)img.size();
    a.wt_doubles = WT_DOUBLES; a.smoother = h->em_smoother;
    a.l = l; a.w = w; a.lvsq = lvsq; a.p_vl = p_vl; a.cur = cur;
    a.assoc = full ? (const long long*)assoc : nullptr;
    a.max_stdd = max_stdd; a.s_thresh = s_thresh;
    a.vp_out = vp_out; a.s_out = s_out; a.err_out = err_out; a.max_err_out = max_err_out;
    a.removed_out = (int*)removed_out; a.valid_out = (int*)valid_out;
    return launch(h, a, img, slot, 2, EM_LDS_BYTES, "vpk_mstep_batch: records");
}

int vpk_init_vps_batch(vpk_handle* h, int batch, const float* cnn, const uint8_t* sphere, int sphere_size, int num_max,
                       double* v0_out, int32_t* m0_out, float* weights_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_init_vps_batch: batch < 0");
    if (batch == 0) return VPK_OK;
    if (!cnn || !sphere || !v0_out || !m0_out || num_max < 1 || num_max > MAXM || sphere_size < GRIDN)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_init_vps_batch: bad argument");
    EmstepArgs a = {};
    a.op = EMSTEP_INIT;
    a.count = batch;
    a.wt_doubles = WT_DOUBLES;
    a.cnn = cnn; a.sphere = sphere; a.ssize = sphere_size; a.num_max = num_max;
    a.v0_out = v0_out; a.m0_out = (int*)m0_out; a.weights_out = weights_out;
    return launch(h, a, std::vector<EmstepImage>(), 0, 2, EM_LDS_BYTES, "vpk_init_vps_batch");
}

}  // extern "C"
