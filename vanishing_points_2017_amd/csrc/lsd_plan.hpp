// lsd_plan.hpp -- what vpk_lsd_detect_batch (vpk_lsd_gpu.hip) decides on the host before it launches anything: the rules
// a batch's images are held to, every image's slice of the workspace, and the split of the batch into chunks whose
// workspace stays under a limit.  Plain C++ without a HIP include: tests/hostsim/sim_lsd_plan.cpp compiles it for the CPU
// tests (tests/test_lsd_plan.py).
//
// A chunk's workspace: one Meta per image, then the images one after the other, every array 256-aligned, in the order
// aux (xs * h doubles), scaled, ang, grad (xs * ys doubles each), order (ints), reg (Pt), used (bytes); aux and scaled
// only when the scale is not 1.  Every chunk starts at the workspace's first byte: the chunks run one after the other.
#ifndef VPK_LSD_PLAN_HPP_
#define VPK_LSD_PLAN_HPP_

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/vpk.h"
#include "lsd_device.hpp"

namespace vpk_lsd {

constexpr int MAX_CHUNK_IMAGES = 4096;
constexpr size_t DEFAULT_WS_LIMIT = (size_t)4 << 30;
constexpr long long MAX_DIM = 1 << 20;            // input or scaled side
constexpr long long MAX_SCALED_PIXELS = 1 << 30;  // seeds are packed as y * xs + x into an int

struct ImgDesc {
    long long in_off;                             // first pixel in `images`
    long long aux, scaled, ang, grad, order, reg, used;   // byte offsets into the chunk's workspace
    int w, h, xs, ys;
    int b;                                        // index in the batch
    int min_reg;
    double logNT;
};

struct Meta {                                     // per image of a chunk, zeroed before it
    unsigned long long max_grad;                  // bits of a non-negative double: integer max = double max
    int n_seeds;
    int pad;
};

inline long long align256(long long v) { return (v + 255) & ~255LL; }

enum PlanRule {                                   // checked per image, in this order
    PLAN_OK = 0,
    PLAN_SIDE,                                    // width or height below 8
    PLAN_OFFSETS,                                 // pix_offsets negative or not width * height apart
    PLAN_DIM,                                     // an input or scaled side beyond MAX_DIM
    PLAN_PIXELS,                                  // a scaled image beyond MAX_SCALED_PIXELS
};

// the code the driver returns for a rule: malformed arguments are VPK_ERR_ARG, the two size limits VPK_ERR_LIMIT
inline int plan_code(PlanRule r) {
    return r == PLAN_OK ? VPK_OK : r == PLAN_DIM || r == PLAN_PIXELS ? VPK_ERR_LIMIT : VPK_ERR_ARG;
}

struct Plan {
    PlanRule rule = PLAN_OK;
    int image = -1;                               // the first image that fails `rule`
    std::vector<ImgDesc> desc;                    // per image, workspace offsets final
    std::vector<int> starts;                      // chunk c holds the images [starts[c], starts[c + 1])
    size_t ws_bytes = 0;                          // the largest chunk's workspace
    int max_c = 0;                                // Gaussian weights are needed for output coordinates 0 .. max_c - 1
};

// dims: width, height per image; pix_offsets: batch + 1; limit: bytes of workspace per chunk, 0 for the default.  A chunk
// takes consecutive images while its workspace stays under the limit, and at least one.
inline Plan plan_batch(int batch, const int32_t* dims, const int64_t* pix_offsets, double scale, size_t limit) {
    Plan p;
    const double prob = make_params(scale).p;
    p.desc.resize((size_t)batch);
    std::vector<long long> bytes((size_t)batch);
    auto fail = [&p](PlanRule r, int b) {
        p.rule = r;
        p.image = b;
        return p;
    };
    for (int b = 0; b < batch; ++b) {
        const int w = dims[2 * b], ht = dims[2 * b + 1];
        if (w < 8 || ht < 8) return fail(PLAN_SIDE, b);
        if (pix_offsets[b + 1] - pix_offsets[b] != (int64_t)w * ht || pix_offsets[b] < 0) return fail(PLAN_OFFSETS, b);
        if (w > MAX_DIM || ht > MAX_DIM || !((double)w * scale <= (double)MAX_DIM) || !((double)ht * scale <= (double)MAX_DIM))
            return fail(PLAN_DIM, b);
        int xs, ys;
        scaled_size(w, ht, scale, xs, ys);
        const long long P = (long long)xs * ys;
        if (P > MAX_SCALED_PIXELS || xs < 1 || ys < 1) return fail(PLAN_PIXELS, b);
        ImgDesc& d = p.desc[(size_t)b];           // value-initialised: aux and scaled stay 0 at scale 1
        d.in_off = pix_offsets[b];
        d.w = w; d.h = ht; d.xs = xs; d.ys = ys; d.b = b;
        d.logNT = log_nt(xs, ys);
        d.min_reg = min_reg_size(d.logNT, prob);
        long long o = 0;                          // offsets from the image's first byte; the chunk's base comes below
        if (scale != 1.0) {
            d.aux = o; o += align256((long long)xs * ht * 8);
            d.scaled = o; o += align256(P * 8);
            p.max_c = xs > p.max_c ? xs : p.max_c;
            p.max_c = ys > p.max_c ? ys : p.max_c;
        }
        d.ang = o; o += align256(P * 8);
        d.grad = o; o += align256(P * 8);
        d.order = o; o += align256(P * 4);
        d.reg = o; o += align256(P * 8);
        d.used = o; o += align256(P);
        bytes[(size_t)b] = o;
    }
    if (!limit) limit = DEFAULT_WS_LIMIT;
    int b = 0;
    while (b < batch) {
        const int s = b;
        long long used = 0;
        while (b < batch && b - s < MAX_CHUNK_IMAGES) {
            const long long meta = align256((long long)(b - s + 1) * sizeof(Meta));
            if (b > s && meta + used + bytes[(size_t)b] > (long long)limit) break;
            used += bytes[(size_t)b];
            ++b;
        }
        p.starts.push_back(s);
        long long base = align256((long long)(b - s) * sizeof(Meta));
        for (int k = s; k < b; ++k) {
            ImgDesc& d = p.desc[(size_t)k];
            if (scale != 1.0) { d.aux += base; d.scaled += base; }
            d.ang += base; d.grad += base; d.order += base; d.reg += base; d.used += base;
            base += bytes[(size_t)k];
        }
        if ((size_t)base > p.ws_bytes) p.ws_bytes = (size_t)base;
    }
    p.starts.push_back(batch);
    return p;
}

}  // namespace vpk_lsd

#endif
