// sim_trainset.cpp -- TEST-ONLY host build of the per-element rules of the device-resident training set
// (csrc/trainset_device.hpp): the counter-based draws, the affine map of a line and of a VP, the label cell and the batch
// slot search, compiled with g++ for tests/test_trainset.py.
#include "../../vanishing_points_2017_amd/csrc/trainset_device.hpp"

extern "C" {

// u_k, k = 0..K-1, of slot b at an iteration
void sim_trainset_draws(unsigned long long seed, unsigned long long iteration, unsigned b, int K, double* out) {
    const uint64_t key = vpk_trainset::draw_key(seed, iteration, b);
    for (int k = 0; k < K; ++k) out[k] = vpk_trainset::draw(key, (uint64_t)k);
}

void sim_trainset_order_keys(unsigned long long seed, unsigned long long epoch, long long n, unsigned long long* out) {
    for (long long i = 0; i < n; ++i) out[i] = vpk_trainset::order_key(seed, epoch, (uint64_t)i);
}

// n rows: h (6), l (3), v (3) -> m (3), w (3), one transform per row
void sim_trainset_transform(long long n, const double* h, const double* l, const double* v, double* m, double* w) {
    for (long long i = 0; i < n; ++i) {
        vpk_trainset::transform_line(h + 6 * i, l + 3 * i, m + 3 * i);
        vpk_trainset::transform_vp(h + 6 * i, v + 3 * i, w + 3 * i);
    }
}

void sim_trainset_cells(long long n, const double* v, int gh, int gw, int* out) {
    for (long long i = 0; i < n; ++i) out[i] = vpk_trainset::label_cell(v + 3 * i, gh, gw);
}

int sim_trainset_valid(const double* h) { return vpk_trainset::affine_valid(h) ? 1 : 0; }

void sim_trainset_slots(const long long* off, int B, long long total, int* out) {
    for (long long t = 0; t < total; ++t) out[t] = vpk_trainset::slot_of(off, B, t);
}

}  // extern "C"
