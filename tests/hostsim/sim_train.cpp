// sim_train.cpp -- TEST-ONLY host build of the per-element functions of the dense head's training step
// (csrc/train_device.hpp): the loss and its gradient, the SGD update of one element, the learning-rate policy and the
// dropout mask hash, compiled with g++ for tests/test_train.py.
#include "../../vanishing_points_2017_amd/csrc/train_device.hpp"

extern "C" {

void sim_train_loss(long long n, const float* z, const float* t, float inv_b, float* loss, float* sig, float* grad) {
    for (long long i = 0; i < n; ++i) {
        loss[i] = vpk_train::loss_term(z[i], t[i]);
        sig[i] = vpk_train::sigmoid(z[i]);
        grad[i] = vpk_train::loss_grad(z[i], t[i], inv_b);
    }
}

float sim_train_learning_rate(float base_lr, float gamma, long long stepsize, long long iteration) {
    return vpk_train::learning_rate(base_lr, gamma, stepsize, iteration);
}

void sim_train_sgd_update(long long n, float* w, float* v, const float* g, float lr_local, float decay_local, float mu) {
    for (long long i = 0; i < n; ++i) vpk_train::sgd_update(w[i], v[i], g[i], lr_local, decay_local, mu);
}

// the B x H keep mask of `layer` at `iteration`, as the step generates it when it is given none
void sim_train_mask(unsigned long long seed, unsigned long long iteration, unsigned layer, int B, int H, float dropout_ratio,
                    unsigned char* out) {
    const uint32_t thr = vpk_train::mask_threshold(dropout_ratio);
    for (int b = 0; b < B; ++b) {
        const uint64_t key = vpk_train::mask_key(seed, iteration, layer, (uint32_t)b);
        for (int j = 0; j < H; ++j) out[(size_t)b * H + j] = vpk_train::mask_bit(key, (uint32_t)j, thr);
    }
}

}  // extern "C"
