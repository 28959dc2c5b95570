// batch_args.hpp -- the rules a ragged batch's host arguments are held to before anything is launched: offsets (batch + 1
// int64 on the host; image b holds [off[b], off[b + 1])) of lines, of VPs and of per-image N_b x N_b matrix slots.  Shared by
// the drivers vpk_vpset.hip, vpk_emstep.hip, vpk_estep.hip and vpk_lines.hip, which turn the rule that failed into their own
// vpk_fail code and text.  Plain C++ without a HIP include: tests/hostsim/sim_batch_args.cpp compiles it for the CPU tests.
#ifndef VPK_BATCH_ARGS_HPP_
#define VPK_BATCH_ARGS_HPP_

#include <stdint.h>

#include "../../include/vpk.h"

namespace vpk {

enum BatchRule {
    BATCH_OK = 0,
    BATCH_EMPTY,     // batch == 0: nothing to launch, not an error
    BATCH_NEGATIVE,  // batch < 0
    BATCH_NULL,      // an offsets array is missing
    BATCH_OFFSETS,   // off[0] < 0, a step down, or an image past the driver's index range
    BATCH_VPS,       // an image has more VPs than the driver's limit
    BATCH_LINES,     // an image has more lines than the driver's limit
    BATCH_SLOT,      // a matrix slot starts below 0 or holds less than N_b^2 elements
};

constexpr long long BATCH_NO_LIMIT = INT64_MAX;

// the code a driver returns for a rule: the two limits are VPK_ERR_LIMIT, every other failure VPK_ERR_ARG
inline int batch_code(BatchRule r) {
    return r == BATCH_OK || r == BATCH_EMPTY ? VPK_OK : r == BATCH_VPS || r == BATCH_LINES ? VPK_ERR_LIMIT : VPK_ERR_ARG;
}

// offsets rise from a value >= 0 and no image is larger than index_max; *largest: the largest image
inline BatchRule batch_offsets(int batch, const int64_t* off, long long* largest, long long index_max = BATCH_NO_LIMIT) {
    *largest = 0;
    if (off[0] < 0) return BATCH_OFFSETS;
    for (int b = 0; b < batch; ++b) {
        const long long n = off[b + 1] - off[b];
        if (n < 0 || n > index_max) return BATCH_OFFSETS;
        if (n > *largest) *largest = n;
    }
    return BATCH_OK;
}

// the line and VP offsets of one batch, in the order the drivers report: batch, pointers, offsets, VP limit, line limit
inline BatchRule batch_pair(int batch, const int64_t* line_off, const int64_t* vp_off, long long max_lines, long long max_vps) {
    if (batch < 0) return BATCH_NEGATIVE;
    if (batch == 0) return BATCH_EMPTY;
    if (!line_off || !vp_off) return BATCH_NULL;
    long long nmax, mmax;
    if (batch_offsets(batch, line_off, &nmax) || batch_offsets(batch, vp_off, &mmax)) return BATCH_OFFSETS;
    return mmax > max_vps ? BATCH_VPS : nmax > max_lines ? BATCH_LINES : BATCH_OK;
}

// slot_off (lsim_offsets, mat_offsets) leaves image b at least N_b^2 elements; the slots may have gaps between them
inline BatchRule batch_slots(int batch, const int64_t* off, const int64_t* slot_off) {
    for (int b = 0; b < batch; ++b) {
        const long long n = off[b + 1] - off[b];
        if (slot_off[b] < 0 || slot_off[b + 1] - slot_off[b] < n * n) return BATCH_SLOT;
    }
    return BATCH_OK;
}

}  // namespace vpk

#endif
