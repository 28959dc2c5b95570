// vpk_estep.hip -- the E-step outside the EM, batched: vpk_estep_batch (see include/vpk.h).  calc_probabilities after its
// prior, with the three distance measures, on caller-supplied lines, VPs and variances.  The kernel body is
// estep_device.hpp's.  Compiled with -ffp-contract=off like the EM unit, whose per-pair expression the "angle" measure
// restates.
#include "estep_device.hpp"
#include "batch_args.hpp"
#include "vpk_internal.hpp"

#include <vector>

using namespace vpk;

namespace {

// one workgroup (one wave) per tile of ESTEP_TILE lines of one image, or per (tile, VP chunk) when the launch is split
template <int MEASURE> __global__ __launch_bounds__(ESTEP_TILE) void estep_batch_kernel(EstepArgs a) {
    estep_block<MEASURE>(a, (long long)block_id());
}

}  // namespace

extern "C" {

int vpk_estep_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets, const double* lp,
                    const double* l, const double* v, const double* s, const double* p_v, int measure,
                    double* s_floored_out, double* lvsq_out, double* p_lv_out, double* p_l_out, double* p_vl_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0 || (measure != VPK_DIST_ANGLE && measure != VPK_DIST_DOTPROD && measure != VPK_DIST_AREA))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_estep_batch: bad batch or unknown measure");
    const BatchRule r = batch_pair(batch, line_offsets, vp_offsets, BATCH_NO_LIMIT, BATCH_NO_LIMIT);   // any N_b, any M_b
    if (r == BATCH_EMPTY) return VPK_OK;
    if (r) return vpk_fail(h, VPK_ERR_ARG, r == BATCH_NULL ? "vpk_estep_batch: null offsets" : "vpk_estep_batch: offsets must not decrease");
    const bool chain = p_l_out || p_vl_out;
    const bool split = !chain;
    // header: [line_off | vp_off | mat_off | blk_off], batch + 1 each
    const size_t B1 = (size_t)batch + 1;
    std::vector<int64_t> hdr(4 * B1);
    int64_t mat = 0, blk = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = line_offsets[b + 1] - line_offsets[b], m = vp_offsets[b + 1] - vp_offsets[b];
        hdr[b] = line_offsets[b]; hdr[B1 + b] = vp_offsets[b]; hdr[2 * B1 + b] = mat; hdr[3 * B1 + b] = blk;
        if (n > 0 && m > 0x7fffffffLL * ESTEP_CHUNK) return vpk_fail(h, VPK_ERR_ARG, "vpk_estep_batch: an image has too many VPs");
        mat += n * m;
        blk += estep_image_blocks(n, m, split);
        if (blk > 0x7fffffffLL) return vpk_fail(h, VPK_ERR_ARG, "vpk_estep_batch: the batch is too large for one launch");
    }
    hdr[batch] = line_offsets[batch]; hdr[B1 + batch] = vp_offsets[batch]; hdr[2 * B1 + batch] = mat; hdr[3 * B1 + batch] = blk;
    if (blk == 0 || (!s_floored_out && !lvsq_out && !p_lv_out && !chain)) return VPK_OK;
    if (!lp || !v || !s || (measure == VPK_DIST_DOTPROD && !l) || (chain && !p_v))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_estep_batch: null buffer");
    VPK_HIP(h, hipSetDevice(h->device));
    const int rc = vpk_stage_upload(h, h->estep_hdr, hdr.data(), hdr.size() * sizeof(int64_t), "vpk_estep_batch: header");
    if (rc) return rc;
    EstepArgs a = {};
    a.batch = batch;
    a.split = split ? 1 : 0;
    a.line_off = (cglp)h->estep_hdr.dev;
    a.vp_off = a.line_off + B1; a.mat_off = a.line_off + 2 * B1; a.blk_off = a.line_off + 3 * B1;
    a.lp = (cgdp)lp; a.l = (cgdp)l; a.v = (cgdp)v; a.s = (cgdp)s; a.p_v = (cgdp)p_v;
    a.s_out = (gdp)s_floored_out; a.lvsq_out = (gdp)lvsq_out; a.p_lv_out = (gdp)p_lv_out; a.p_l_out = (gdp)p_l_out;
    a.p_vl_out = (gdp)p_vl_out;
    const dim3 grid((unsigned)blk), block(ESTEP_TILE);
    if (measure == VPK_DIST_ANGLE)
        hipLaunchKernelGGL(estep_batch_kernel<VPK_DIST_ANGLE>, grid, block, ESTEP_LDS_BYTES, h->stream, a);
    else if (measure == VPK_DIST_DOTPROD)
        hipLaunchKernelGGL(estep_batch_kernel<VPK_DIST_DOTPROD>, grid, block, ESTEP_LDS_BYTES, h->stream, a);
    else
        hipLaunchKernelGGL(estep_batch_kernel<VPK_DIST_AREA>, grid, block, ESTEP_LDS_BYTES, h->stream, a);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // extern "C"
