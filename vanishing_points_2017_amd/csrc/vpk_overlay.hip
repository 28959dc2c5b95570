// vpk_overlay.hip -- result overlays, batched: coloured segments blended into a ragged batch of RGB images
// (vpk_overlay_lines_batch) and discs blended into a batch of square panels (vpk_overlay_markers_batch; see include/vpk.h).
// The kernel body is overlay_device.hpp's overlay_tile; the renderer is specified in DESIGN section 7d.  Compiled with
// -ffp-contract=off: the distance is line_device.hpp's.
#include "overlay_device.hpp"
#include "vpk_internal.hpp"

#include <vector>

using namespace vpk;

namespace {

// the block index is image-major: tiles_per_image blocks for every image, those past an image's tiles return at once
template <bool DISC>
__global__ __launch_bounds__(OV_THREADS) void overlay_kernel(OverlayArgs a, int tiles_per_image) {
    overlay_tile<DISC>(a, block_id() / tiles_per_image, block_id() % tiles_per_image);
}

// dims: batch x (W, H).  Checks everything the host can see, uploads the header, launches; nothing is launched on an error.
template <bool DISC>
int overlay_launch(vpk_handle* h, const char* who, int batch, const int64_t* dims, const int64_t* pix_offsets, unsigned char* rgb,
                   const int64_t* prim_offsets, const double* geom, const uint8_t* rgba, const double* width) {
    char msg[160];
    auto bad = [&](const char* what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return vpk_fail(h, VPK_ERR_ARG, msg);
    };
    if (!pix_offsets || !prim_offsets) return bad("null offsets");
    if (pix_offsets[0] < 0 || prim_offsets[0] < 0) return bad("negative offset");
    long long tmax = 0, pmax = 0;
    for (int b = 0; b < batch; ++b) {
        const long long w = dims[2 * b], ht = dims[2 * b + 1];
        if (w < 1 || ht < 1 || w > 0x7fffffffLL || ht > 0x7fffffffLL) return bad("an image side below 1");
        if (ht > 0x7fffffffffffffffLL / 3 / w || pix_offsets[b + 1] - pix_offsets[b] < 3 * w * ht)
            return bad("pix_offsets must rise by at least 3 W H bytes per image");
        const long long p = prim_offsets[b + 1] - prim_offsets[b];
        if (p < 0 || p > 0x7fffffffLL) return bad("primitive offsets must not decrease");
        const long long t = ((w + OV_TILE - 1) / OV_TILE) * ((ht + OV_TILE - 1) / OV_TILE);
        if (t > 0x7fffffffLL) return bad("image too large for one launch");
        if (p > 0 && t > tmax) tmax = t;
        if (p > pmax) pmax = p;
    }
    if (pmax == 0) return VPK_OK;
    if (!rgb || !geom || !rgba || !width) return bad("null buffer");
    if (tmax * batch > 0x7fffffffLL) return bad("batch x tiles too large for one launch");
    VPK_HIP(h, hipSetDevice(h->device));
    const size_t nb = (size_t)batch;
    std::vector<int64_t> hdr(2 * nb + 2 * (nb + 1));
    for (size_t b = 0; b < 2 * nb; ++b) hdr[b] = dims[b];
    for (size_t b = 0; b <= nb; ++b) { hdr[2 * nb + b] = pix_offsets[b]; hdr[3 * nb + 1 + b] = prim_offsets[b]; }
    const int rc = vpk_stage_upload(h, h->overlay_hdr, hdr.data(), hdr.size() * sizeof(int64_t), who);
    if (rc) return rc;
    OverlayArgs a = {};
    a.dims = (cglp)h->overlay_hdr.dev;
    a.pix_offsets = a.dims + 2 * nb;
    a.prim_offsets = a.pix_offsets + nb + 1;
    a.geom = (cgdp)geom;
    a.width = (cgdp)width;
    a.rgba = (cgup)(const void*)rgba;
    a.rgb = (gbp)rgb;
    hipLaunchKernelGGL(overlay_kernel<DISC>, dim3((unsigned)(tmax * batch)), dim3(OV_THREADS), OV_LDS_BYTES, h->stream, a, (int)tmax);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // namespace

extern "C" {

int vpk_overlay_lines_batch(vpk_handle* h, int batch, const int32_t* dims, const int64_t* pix_offsets, uint8_t* rgb_inout,
                            const int64_t* seg_offsets, const double* seg_px, const uint8_t* seg_rgba, const double* seg_width) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_overlay_lines_batch: negative batch");
    if (batch == 0) return VPK_OK;
    if (!dims) return vpk_fail(h, VPK_ERR_ARG, "vpk_overlay_lines_batch: null dims");
    std::vector<int64_t> d(2 * (size_t)batch);
    for (size_t b = 0; b < d.size(); ++b) d[b] = dims[b];
    return overlay_launch<false>(h, "vpk_overlay_lines_batch", batch, d.data(), pix_offsets, rgb_inout, seg_offsets, seg_px, seg_rgba,
                                 seg_width);
}

int vpk_overlay_markers_batch(vpk_handle* h, int batch, const int32_t* sizes, const int64_t* pix_offsets, uint8_t* rgb_inout,
                              const int64_t* mark_offsets, const double* mark_xy, const uint8_t* mark_rgba,
                              const double* mark_diameter) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_overlay_markers_batch: negative batch");
    if (batch == 0) return VPK_OK;
    if (!sizes) return vpk_fail(h, VPK_ERR_ARG, "vpk_overlay_markers_batch: null sizes");
    std::vector<int64_t> d(2 * (size_t)batch);
    for (int b = 0; b < batch; ++b) d[2 * (size_t)b] = d[2 * (size_t)b + 1] = sizes[b];
    return overlay_launch<true>(h, "vpk_overlay_markers_batch", batch, d.data(), pix_offsets, rgb_inout, mark_offsets, mark_xy,
                                mark_rgba, mark_diameter);
}

}  // extern "C"
