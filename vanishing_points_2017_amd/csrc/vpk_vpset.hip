// vpk_vpset.hip -- VP set maintenance outside the EM, batched: vpk_vp_line_counts_batch, vpk_vp_split_batch and
// vpk_vp_merge_batch (see include/vpk.h).  One workgroup per image runs one operation on the caller's VP set through the
// EM workgroup's own device functions (vpset_device.hpp).  Compiled with -ffp-contract=off like the EM unit.
#include "vpset_device.hpp"
#include "batch_args.hpp"
#include "vpk_internal.hpp"

#include <algorithm>
#include <vector>

using namespace vpk;

namespace {

constexpr int VPSET_THREADS = 512;                     // the EM workgroup's shape: the phase functions are tuned for 8 waves
constexpr long long VPSET_NMAX = 32768;                // cluster2 indexes an n x n matrix with ints

// one kernel per distance measure, as vpk_em.hip and vpk_estep.hip have them: no run-time branch in a pair loop
template <int MEASURE> __global__ __launch_bounds__(VPSET_THREADS) void vpset_kernel(VpsetArgs a) { vpset_run<MEASURE>(a); }

typedef void (*vpset_kernel_t)(VpsetArgs);
vpset_kernel_t kernel_of(int measure) {
    return measure == VPK_DIST_DOTPROD ? vpset_kernel<VPK_DIST_DOTPROD>
         : measure == VPK_DIST_AREA ? vpset_kernel<VPK_DIST_AREA> : vpset_kernel<VPK_DIST_ANGLE>;
}
bool known_measure(int measure) { return measure == VPK_DIST_ANGLE || measure == VPK_DIST_DOTPROD || measure == VPK_DIST_AREA; }

// header: [line_off | vp_off | mat_off | ws_off] (batch + 1 each) and the active list; returns the number of active images
int build_header(int batch, const int64_t* line_off, const int64_t* vp_off, int op, std::vector<int64_t>& hdr, long long* ws_doubles,
                 const int64_t* lsim_off = nullptr, long long slot = 0) {
    const size_t B1 = (size_t)batch + 1;
    hdr.assign(5 * B1, 0);
    int64_t mat = 0, ws = 0;
    int active = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = line_off[b + 1] - line_off[b], m = vp_off[b + 1] - vp_off[b];
        hdr[b] = line_off[b]; hdr[B1 + b] = vp_off[b]; hdr[2 * B1 + b] = lsim_off ? lsim_off[b] : mat; hdr[3 * B1 + b] = ws;
        mat += n * m;
        if (n > 0 && m > 0) {
            hdr[4 * B1 + active++] = b;
            if (op == VPSET_MERGE) { ws += slot; continue; }   // one EM slot (em_layout.hpp)
            // counts: N ints; split: cl N x N, directions 3 N, assoc + idx 4 N ints (vpset_device.hpp)
            const int64_t need = op == VPSET_COUNTS ? (n + 1) / 2 : n * n + 3 * n + 2 * n;
            ws += (need + 31) / 32 * 32;
        }
    }
    hdr[batch] = line_off[batch]; hdr[B1 + batch] = vp_off[batch]; hdr[2 * B1 + batch] = mat; hdr[3 * B1 + batch] = ws;
    *ws_doubles = ws;
    return active;
}

int launch(vpk_handle* h, int measure, int batch, const std::vector<int64_t>& hdr, int active, long long ws_doubles, VpsetArgs& a,
           const char* who) {
    VPK_HIP(h, hipSetDevice(h->device));
    if ((size_t)ws_doubles * 8 > h->total_mem / 2) return vpk_fail(h, VPK_ERR_LIMIT, "vpset: the batch's workspace exceeds half of the device memory");
    if (!h->vpset_ready) {
        for (int m : {VPK_DIST_ANGLE, VPK_DIST_DOTPROD, VPK_DIST_AREA})
            VPK_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel_of(m)), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)EM_LDS_BYTES));
        h->vpset_ready = true;
    }
    int rc = vpk_reserve(h, &h->vpset_ws, &h->vpset_ws_bytes, (size_t)(ws_doubles > 0 ? ws_doubles : 32) * 8, "hipMalloc(vpset workspace)");
    if (rc) return rc;
    rc = vpk_stage_upload(h, h->vpset_hdr, hdr.data(), hdr.size() * sizeof(int64_t), who);
    if (rc) return rc;
    const size_t B1 = (size_t)batch + 1;
    cgllp d = (cgllp)h->vpset_hdr.dev;
    a.line_off = d; a.vp_off = d + B1; a.mat_off = d + 2 * B1; a.ws_off = d + 3 * B1; a.active = d + 4 * B1;
    a.ws = (gdp)h->vpset_ws;
    a.wt_doubles = WT_DOUBLES;
    hipLaunchKernelGGL(kernel_of(measure), dim3((unsigned)active), dim3(VPSET_THREADS), EM_LDS_BYTES, h->stream, a);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

// the checks the three entries share; *done = nothing to launch
int check_batch(vpk_handle* h, int batch, const int64_t* line_off, const int64_t* vp_off, const char* who, bool* done) {
    const BatchRule r = batch_pair(batch, line_off, vp_off, VPSET_NMAX, MAXM);
    *done = r != BATCH_OK;
    if (r == BATCH_OK || r == BATCH_EMPTY) return VPK_OK;
    return vpk_fail(h, batch_code(r), r == BATCH_VPS ? "vpset: an image has more than 64 VPs"
                                      : r == BATCH_LINES ? "vpset: an image has more than 32768 lines" : who);
}

}  // namespace

extern "C" {

int vpk_vp_line_counts_batch_measure(vpk_handle* h, int measure, int batch, const int64_t* line_offsets, const int64_t* vp_offsets,
                                     const double* lp, const double* l, const double* v, const double* s, const double* metric,
                                     const double* lweights, double thresh, const int64_t* vp_assoc_in, double* counts_out,
                                     double* counts_w_out, int64_t* vp_assoc_out) {
    if (!h) return VPK_ERR_ARG;
    if (!known_measure(measure)) return vpk_fail(h, VPK_ERR_ARG, "vpk_vp_line_counts_batch_measure: unknown measure");
    if (measure == VPK_DIST_DOTPROD && !l) return vpk_fail(h, VPK_ERR_ARG, "vpk_vp_line_counts_batch_measure: \"dotprod\" reads l");
    bool done;
    int rc = check_batch(h, batch, line_offsets, vp_offsets, "vpk_vp_line_counts_batch: bad batch or offsets", &done);
    if (rc || done) return rc;
    std::vector<int64_t> hdr;
    long long ws;
    const int active = build_header(batch, line_offsets, vp_offsets, VPSET_COUNTS, hdr, &ws);
    if (active == 0) return VPK_OK;
    if (!lp || !v || !s || !lweights || (!metric && !vp_assoc_in) || !counts_out || !counts_w_out || !vp_assoc_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_vp_line_counts_batch: null buffer");
    VpsetArgs a = {};
    a.op = VPSET_COUNTS;
    a.lp = (cgdp)lp; a.l = (cgdp)l; a.v = (cgdp)v; a.s = (cgdp)s; a.w = (cgdp)metric; a.lweight = (cgdp)lweights;
    a.assoc_in = (cgllp)vp_assoc_in;
    a.thresh = thresh;
    a.counts = (gdp)counts_out; a.counts_w = (gdp)counts_w_out; a.assoc_out = (gllp)vp_assoc_out;
    return launch(h, measure, batch, hdr, active, ws, a, "vpk_vp_line_counts_batch: header");
}

int vpk_vp_line_counts_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets, const double* lp,
                             const double* v, const double* s, const double* metric, const double* lweights, double thresh,
                             const int64_t* vp_assoc_in, double* counts_out, double* counts_w_out, int64_t* vp_assoc_out) {
    return vpk_vp_line_counts_batch_measure(h, VPK_DIST_ANGLE, batch, line_offsets, vp_offsets, lp, nullptr, v, s, metric, lweights, thresh,
                                            vp_assoc_in, counts_out, counts_w_out, vp_assoc_out);
}

int vpk_vp_split_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets, const double* lp,
                       const double* l, const double* v, const double* s, const double* w, const double* lweight,
                       const double* langles, double min_diff, double* v_out, double* s_out, int32_t* m_out,
                       int32_t* split_out, uint32_t* flags_out, int32_t* labels_out) {
    if (!h) return VPK_ERR_ARG;
    bool done;
    int rc = check_batch(h, batch, line_offsets, vp_offsets, "vpk_vp_split_batch: bad batch or offsets", &done);
    if (rc || done) return rc;
    std::vector<int64_t> hdr;
    long long ws;
    const int active = build_header(batch, line_offsets, vp_offsets, VPSET_SPLIT, hdr, &ws);
    if (active == 0) return VPK_OK;
    if (!lp || !l || !v || !s || !w || !lweight || !langles || !v_out || !s_out || !m_out || !split_out || !flags_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_vp_split_batch: null buffer");
    VpsetArgs a = {};
    a.op = VPSET_SPLIT;
    a.lp = (cgdp)lp; a.l = (cgdp)l; a.v = (cgdp)v; a.s = (cgdp)s; a.w = (cgdp)w; a.lweight = (cgdp)lweight;
    a.langle = (cgdp)langles;
    a.thresh = min_diff;
    a.v_out = (gdp)v_out; a.s_out = (gdp)s_out; a.m_out = (gip)m_out; a.split_out = (gip)split_out;
    a.flags_out = (VPK_GLOBAL unsigned*)flags_out; a.labels_out = (gip)labels_out;
    return launch(h, VPK_DIST_ANGLE, batch, hdr, active, ws, a, "vpk_vp_split_batch: header");
}

int vpk_vp_merge_batch_measure(vpk_handle* h, int measure, int batch, const int64_t* line_offsets, const int64_t* vp_offsets,
                               const double* lp, const double* l, const double* v, const double* s, const double* lweight,
                               const int64_t* lsim_offsets, const double* lsim, double wbias, const float* prior_weights,
                               double prior_sigma, double thresh, double max_stdd, double* v_out, double* s_out, int32_t* m_out,
                               int32_t* keep_out, uint32_t* flags_out) {
    if (!h) return VPK_ERR_ARG;
    if (!known_measure(measure)) return vpk_fail(h, VPK_ERR_ARG, "vpk_vp_merge_batch_measure: unknown measure");
    bool done;
    int rc = check_batch(h, batch, line_offsets, vp_offsets, "vpk_vp_merge_batch: bad batch or offsets", &done);
    if (rc || done) return rc;
    if (!lsim_offsets || !(prior_sigma > 0)) return vpk_fail(h, VPK_ERR_ARG, "vpk_vp_merge_batch: null lsim_offsets or sigma not > 0");
    if (batch_slots(batch, line_offsets, lsim_offsets))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_vp_merge_batch: lsim_offsets leave image b less than N_b^2 elements");
    long long nmax = 0, mmax = 0;
    for (int b = 0; b < batch; ++b) {
        const long long n = line_offsets[b + 1] - line_offsets[b], m = vp_offsets[b + 1] - vp_offsets[b];
        if (n > 0 && m > 0) { nmax = std::max(nmax, n); mmax = std::max(mmax, m); }
    }
    const EmLayout L = em_layout((int)nmax, (int)em_align((size_t)std::max(mmax, 1LL), 8), VPSET_THREADS / 64, true, false);
    std::vector<int64_t> hdr;
    long long ws;
    const int active = build_header(batch, line_offsets, vp_offsets, VPSET_MERGE, hdr, &ws, lsim_offsets, (long long)L.total_doubles);
    if (active == 0) return VPK_OK;
    if (!lp || !l || !v || !s || !lweight || !lsim || !prior_weights || !v_out || !s_out || !m_out || !keep_out || !flags_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_vp_merge_batch: null buffer");
    VpsetArgs a = {};
    a.op = VPSET_MERGE;
    a.lp = (cgdp)lp; a.l = (cgdp)l; a.v = (cgdp)v; a.s = (cgdp)s; a.lweight = (cgdp)lweight; a.lsim = (cgdp)lsim;
    a.L = L;
    a.prior_w = (const VPK_GLOBAL float*)prior_weights; a.prior_sigma = prior_sigma; a.wbias = wbias;
    a.thresh = thresh; a.max_stdd = max_stdd;
    a.v_out = (gdp)v_out; a.s_out = (gdp)s_out; a.m_out = (gip)m_out; a.keep_out = (gip)keep_out;
    a.flags_out = (VPK_GLOBAL unsigned*)flags_out;
    return launch(h, measure, batch, hdr, active, ws, a, "vpk_vp_merge_batch: header");
}

int vpk_vp_merge_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets, const double* lp,
                       const double* l, const double* v, const double* s, const double* lweight, const int64_t* lsim_offsets,
                       const double* lsim, double wbias, const float* prior_weights, double prior_sigma, double thresh,
                       double max_stdd, double* v_out, double* s_out, int32_t* m_out, int32_t* keep_out, uint32_t* flags_out) {
    return vpk_vp_merge_batch_measure(h, VPK_DIST_ANGLE, batch, line_offsets, vp_offsets, lp, l, v, s, lweight, lsim_offsets, lsim, wbias,
                                      prior_weights, prior_sigma, thresh, max_stdd, v_out, s_out, m_out, keep_out, flags_out);
}

}  // extern "C"
