// vpk_frontend.hip -- the image front end around the GPU line segment detector (C-ABI entries vpk_image_prepare_batch and
// vpk_lsd_rows_to_lines): decoded uint8 images -> fit-resize -> fp64 grey levels for vpk_lsd_detect_batch, and its rows ->
// normalised segments and homogeneous lines in the CSR layout of vpk_sphere_raster / vpk_em_batch.  The arithmetic is in
// image_device.hpp.  Three launches, every one grid-wide over the batch (blockIdx.y = image):
//   fe_resize_x       horizontal Lanczos pass, one lane per (output column, input row), every channel; uint8 intermediate
//   fe_resize_y_grey  vertical pass (or a copy when the height is unchanged) fused with the grey conversion, one lane per
//                     output pixel; also writes the resized uint8 image when asked
//   fe_rows_to_lines  one lane per detector row
// The Lanczos weights of every distinct (input size, output size) of an axis are made once per call on the host (glibc
// sin) and uploaded with the descriptors; the passes are integer arithmetic, so the device reproduces the host build
// (tests/hostsim/sim_frontend.cpp) and Pillow byte for byte.
#include "vpk_internal.hpp"

#include <map>
#include <string.h>
#include <utility>

#include "image_device.hpp"

using namespace vpk_img;

namespace {

constexpr int PASS_THREADS = 256;
constexpr int MAX_LAUNCH_IMAGES = 4096;          // grid.y of one launch
constexpr long long MAX_SIDE = 1 << 20;

struct PrepDesc {
    long long in_off;        // first byte of the image in `images`
    long long tmp_off;       // first byte of its horizontal intermediate in the workspace (out_w x in_h x ch)
    long long out_px;        // first pixel of its grey levels
    long long res_off;       // first byte of its resized image
    long long bx, cx, by, cy; // int32 offsets into the weight table: bounds / coefficients of x and of y
    int in_w, in_h, ch, out_w, out_h;
    int kx, ky;              // taps per output index; 0 = the pass is skipped
    int pad;
};

struct RowDesc {
    long long line_off;      // first line of the image in the outputs
    int w, h, n;
    int pad;
};

inline long long align256(long long v) { return (v + 255) & ~255LL; }

inline unsigned pass_blocks(long long total) {
    const long long g = (total + PASS_THREADS - 1) / PASS_THREADS;
    return (unsigned)(g < 1 ? 1 : g < 1024 ? g : 1024);
}

__global__ void __launch_bounds__(PASS_THREADS) fe_resize_x(const PrepDesc* __restrict__ desc, const int32_t* __restrict__ wt,
                                                            const uint8_t* __restrict__ images, uint8_t* __restrict__ tmp) {
    const PrepDesc d = desc[blockIdx.y];
    if (!d.kx) return;
    const long long total = (long long)d.out_w * d.in_h;
    const int32_t* bounds = wt + d.bx;
    const int32_t* coeffs = wt + d.cx;
    for (long long i = (long long)blockIdx.x * PASS_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * PASS_THREADS) {
        const int y = (int)(i / d.out_w), x = (int)(i % d.out_w);
        const int xmin = bounds[2 * x], n = bounds[2 * x + 1];
        const uint8_t* src = images + d.in_off + ((long long)y * d.in_w + xmin) * d.ch;
        uint8_t* dst = tmp + d.tmp_off + i * d.ch;
        for (int c = 0; c < d.ch; ++c) dst[c] = resample_px(src + c, d.ch, n, coeffs + (long long)x * d.kx);
    }
}

__global__ void __launch_bounds__(PASS_THREADS) fe_resize_y_grey(const PrepDesc* __restrict__ desc, const int32_t* __restrict__ wt,
                                                                 const uint8_t* __restrict__ images, const uint8_t* __restrict__ tmp,
                                                                 uint8_t* __restrict__ resized, double* __restrict__ grey) {
    const PrepDesc d = desc[blockIdx.y];
    const long long total = (long long)d.out_w * d.out_h;
    const uint8_t* src = d.kx ? tmp + d.tmp_off : images + d.in_off;    // out_w columns either way
    const long long row = (long long)d.out_w * d.ch;
    const int32_t* bounds = wt + d.by;
    const int32_t* coeffs = wt + d.cy;
    for (long long i = (long long)blockIdx.x * PASS_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * PASS_THREADS) {
        const int y = (int)(i / d.out_w), x = (int)(i % d.out_w);
        uint8_t px[3];
        for (int c = 0; c < d.ch; ++c) {
            if (d.ky) {
                const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
                px[c] = resample_px(src + ymin * row + (long long)x * d.ch + c, row, n, coeffs + (long long)y * d.ky);
            } else {
                px[c] = src[i * d.ch + c];
            }
        }
        if (resized)
            for (int c = 0; c < d.ch; ++c) resized[d.res_off + i * d.ch + c] = px[c];
        grey[d.out_px + i] = d.ch == 3 ? grey_rgb(px[0], px[1], px[2]) : grey_l(px[0]);
    }
}

__global__ void __launch_bounds__(PASS_THREADS) fe_rows_to_lines(const RowDesc* __restrict__ desc, int b0, const double* __restrict__ rows,
                                                                 int max_segments, double* __restrict__ lp, double* __restrict__ l,
                                                                 double* __restrict__ nfa) {
    const RowDesc d = desc[blockIdx.y];
    const long long b = b0 + (long long)blockIdx.y;
    for (int i = blockIdx.x * PASS_THREADS + threadIdx.x; i < d.n; i += gridDim.x * PASS_THREADS) {
        const double* r = rows + (b * max_segments + i) * 7;
        const long long o = d.line_off + i;
        double p[4], q[3];
        row_to_line(r, d.w, d.h, p, q);
        if (lp)
            for (int k = 0; k < 4; ++k) lp[o * 4 + k] = p[k];
        if (l)
            for (int k = 0; k < 3; ++k) l[o * 3 + k] = q[k];
        if (nfa) nfa[o] = r[6];
    }
}

}  // namespace

extern "C" {

int vpk_image_prepare_batch(vpk_handle* h, int batch, const int32_t* dims, const int64_t* in_offsets, const uint8_t* images,
                            const int64_t* out_offsets, uint8_t* resized_out, double* grey_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0 || (batch > 0 && (!dims || !in_offsets || !images || !out_offsets || !grey_out)))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_image_prepare_batch: bad argument");
    if (batch == 0) return VPK_OK;
    std::vector<PrepDesc> desc((size_t)batch);
    std::map<std::pair<int, int>, std::pair<long long, long long>> tables;   // (in, out) -> bounds, coefficients
    std::vector<int32_t> wt;
    std::vector<double> scratch;
    auto table = [&](int in, int out, int& ksize, long long& bo, long long& co) {
        ksize = 0;
        if (in == out) return;                                             // the pass is skipped
        ksize = lanczos_ksize(in, out);
        auto it = tables.find({in, out});
        if (it == tables.end()) {
            const long long b = (long long)wt.size(), c = b + 2LL * out;
            wt.resize((size_t)(c + (long long)out * ksize));
            if (scratch.size() < (size_t)ksize) scratch.resize((size_t)ksize);
            lanczos_coeffs(in, out, ksize, wt.data() + b, wt.data() + c, scratch.data());
            it = tables.emplace(std::make_pair(in, out), std::make_pair(b, c)).first;
        }
        bo = it->second.first;
        co = it->second.second;
    };
    long long tmp_bytes = 0, res_bytes = 0, max_x = 0, max_y = 0;
    for (int b = 0; b < batch; ++b) {
        const int* v = dims + 5 * (long long)b;
        const int in_w = v[0], in_h = v[1], ch = v[2], out_w = v[3], out_h = v[4];
        if (ch != 1 && ch != 3) return vpk_fail(h, VPK_ERR_ARG, "vpk_image_prepare_batch: channels must be 1 or 3");
        if (in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_image_prepare_batch: every side must be >= 1");
        if (in_w > MAX_SIDE || in_h > MAX_SIDE || out_w > MAX_SIDE || out_h > MAX_SIDE)
            return vpk_fail(h, VPK_ERR_LIMIT, "vpk_image_prepare_batch: image side beyond 2^20 pixels");
        if (in_offsets[b] < 0 || in_offsets[b + 1] - in_offsets[b] != (int64_t)in_w * in_h * ch)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_image_prepare_batch: in_offsets do not match in_w * in_h * channels");
        if (out_offsets[b] < 0 || out_offsets[b + 1] - out_offsets[b] != (int64_t)out_w * out_h)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_image_prepare_batch: out_offsets do not match out_w * out_h");
        PrepDesc& d = desc[(size_t)b];
        memset(&d, 0, sizeof(d));
        d.in_off = in_offsets[b];
        d.out_px = out_offsets[b];
        d.res_off = res_bytes;
        d.in_w = in_w; d.in_h = in_h; d.ch = ch; d.out_w = out_w; d.out_h = out_h;
        table(in_w, out_w, d.kx, d.bx, d.cx);
        table(in_h, out_h, d.ky, d.by, d.cy);
        if (d.kx) {
            d.tmp_off = tmp_bytes;
            tmp_bytes += align256((long long)out_w * in_h * ch);
            max_x = (long long)out_w * in_h > max_x ? (long long)out_w * in_h : max_x;
        }
        max_y = (long long)out_w * out_h > max_y ? (long long)out_w * out_h : max_y;
        res_bytes += (long long)out_w * out_h * ch;
    }
    VPK_HIP(h, hipSetDevice(h->device));
    const size_t desc_bytes = (size_t)align256((long long)batch * sizeof(PrepDesc));
    std::vector<unsigned char> hdr(desc_bytes + wt.size() * sizeof(int32_t));
    memcpy(hdr.data(), desc.data(), (size_t)batch * sizeof(PrepDesc));
    if (!wt.empty()) memcpy(hdr.data() + desc_bytes, wt.data(), wt.size() * sizeof(int32_t));
    int rc = vpk_stage_upload(h, h->fe_prep, hdr.data(), hdr.size(), "vpk_image_prepare_batch: header");
    if (rc) return rc;
    if (tmp_bytes) {
        rc = vpk_reserve(h, &h->fe_ws, &h->fe_ws_bytes, (size_t)tmp_bytes, "vpk_image_prepare_batch: workspace");
        if (rc) return rc;
    }
    const PrepDesc* ddesc = (const PrepDesc*)h->fe_prep.dev;
    const int32_t* dwt = (const int32_t*)((unsigned char*)h->fe_prep.dev + desc_bytes);
    uint8_t* tmp = (uint8_t*)h->fe_ws;
    for (int s = 0; s < batch; s += MAX_LAUNCH_IMAGES) {
        const int n = batch - s < MAX_LAUNCH_IMAGES ? batch - s : MAX_LAUNCH_IMAGES;
        if (max_x)
            hipLaunchKernelGGL(fe_resize_x, dim3(pass_blocks(max_x), n), dim3(PASS_THREADS), 0, h->stream, ddesc + s, dwt, images, tmp);
        hipLaunchKernelGGL(fe_resize_y_grey, dim3(pass_blocks(max_y), n), dim3(PASS_THREADS), 0, h->stream, ddesc + s, dwt, images,
                           (const uint8_t*)tmp, resized_out, grey_out);
        VPK_HIP(h, hipGetLastError());
    }
    return VPK_OK;
}

int vpk_lsd_rows_to_lines(vpk_handle* h, int batch, const int32_t* dims, const double* rows, int max_segments,
                          const int64_t* line_offsets, double* lp_out, double* l_out, double* nfa_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0 || max_segments < 0 || (batch > 0 && (!dims || !line_offsets)))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_lsd_rows_to_lines: bad argument");
    if (batch == 0) return VPK_OK;
    std::vector<RowDesc> desc((size_t)batch);
    int max_n = 0;
    if (line_offsets[0] < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_lsd_rows_to_lines: line_offsets[0] < 0");
    for (int b = 0; b < batch; ++b) {
        const int64_t n = line_offsets[b + 1] - line_offsets[b];
        if (n < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_lsd_rows_to_lines: line_offsets decrease");
        if (n > max_segments)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_lsd_rows_to_lines: a line count exceeds max_segments (detect again with a larger buffer)");
        if (dims[2 * b] < 1 || dims[2 * b + 1] < 1) return vpk_fail(h, VPK_ERR_ARG, "vpk_lsd_rows_to_lines: width and height must be >= 1");
        RowDesc& d = desc[(size_t)b];
        memset(&d, 0, sizeof(d));
        d.line_off = line_offsets[b];
        d.w = dims[2 * b];
        d.h = dims[2 * b + 1];
        d.n = (int)n;
        max_n = d.n > max_n ? d.n : max_n;
    }
    if (max_n == 0) return VPK_OK;
    if (!rows) return vpk_fail(h, VPK_ERR_ARG, "vpk_lsd_rows_to_lines: rows is NULL");
    VPK_HIP(h, hipSetDevice(h->device));
    const int rc = vpk_stage_upload(h, h->fe_rows, desc.data(), desc.size() * sizeof(RowDesc), "vpk_lsd_rows_to_lines: header");
    if (rc) return rc;
    const RowDesc* ddesc = (const RowDesc*)h->fe_rows.dev;
    for (int s = 0; s < batch; s += MAX_LAUNCH_IMAGES) {
        const int n = batch - s < MAX_LAUNCH_IMAGES ? batch - s : MAX_LAUNCH_IMAGES;
        hipLaunchKernelGGL(fe_rows_to_lines, dim3(pass_blocks(max_n), n), dim3(PASS_THREADS), 0, h->stream, ddesc + s, s, rows,
                           max_segments, lp_out, l_out, nfa_out);
        VPK_HIP(h, hipGetLastError());
    }
    return VPK_OK;
}

}  // extern "C"
