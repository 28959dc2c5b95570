// sim_batch_args.cpp -- TEST-ONLY host build of csrc/batch_args.hpp: the rules the batch drivers hold their host offsets to,
// callable from the CPU tests (tests/test_batch_args.py).  The header is plain C++, so this needs no hip_sim.hpp.
#include "../../vanishing_points_2017_amd/csrc/batch_args.hpp"

using namespace vpk;

extern "C" {

// the rule (BatchRule); *largest: the largest image where the offsets are well formed
int sim_batch_offsets(int batch, const int64_t* off, long long index_max, long long* largest) {
    return batch_offsets(batch, off, largest, index_max < 0 ? BATCH_NO_LIMIT : index_max);
}

int sim_batch_pair(int batch, const int64_t* line_off, const int64_t* vp_off, long long max_lines, long long max_vps) {
    return batch_pair(batch, line_off, vp_off, max_lines < 0 ? BATCH_NO_LIMIT : max_lines, max_vps < 0 ? BATCH_NO_LIMIT : max_vps);
}

int sim_batch_slots(int batch, const int64_t* off, const int64_t* slot_off) { return batch_slots(batch, off, slot_off); }

int sim_batch_code(int rule) { return batch_code((BatchRule)rule); }

}  // extern "C"
