// train_device.hpp -- the per-element arithmetic of the dense head's training step (vpk_train.hip), for device and host.
//
// The step is train/train_val.prototxt:289-417 (fc6 .. the loss) under train/solver.prototxt: three InnerProduct layers with
// ReLU and Dropout between them, SigmoidCrossEntropyLoss on top, Caffe's SGD solver with momentum, weight decay and the "step"
// learning-rate policy.  Everything here is float32; tests/hostsim/sim_train.cpp compiles these same functions with g++.
#ifndef VPK_TRAIN_DEVICE_HPP_
#define VPK_TRAIN_DEVICE_HPP_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VPK_TRAIN_FN __host__ __device__ inline
#else
#define VPK_TRAIN_FN inline
#endif

namespace vpk_train {

// SigmoidCrossEntropyLoss of one logit z against a label t in [0, 1], in Caffe's stable form
// (sigmoid_cross_entropy_loss_layer: loss -= z (t - [z >= 0]) - log(1 + exp(z - 2 z [z >= 0]))):
//   max(z, 0) - z t + log1p(exp(-|z|))
VPK_TRAIN_FN float loss_term(float z, float t) {
    return (fmaxf(z, 0.0f) - z * t) + log1pf(expf(-fabsf(z)));
}

// sigmoid(z) without overflow on either side: exp is only taken of -|z|
VPK_TRAIN_FN float sigmoid(float z) {
    const float e = expf(-fabsf(z));
    return z >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// d loss / d z of the batch-normalised loss: (sigmoid(z) - t) / B, given inv_b = 1 / B.  Formed from exp(-|z|) and not from
// the rounded sigmoid, so that a saturated unit keeps its small gradient: at z = 20, t = 1 the rounded sigmoid is 1 and
// sigmoid - t would be 0, where the gradient is -2.1e-9 / B.
VPK_TRAIN_FN float loss_grad(float z, float t, float inv_b) {
    const float e = expf(-fabsf(z));
    const float num = z >= 0.0f ? (1.0f - t) - t * e : e * (1.0f - t) - t;
    return num / (1.0f + e) * inv_b;
}

// solver.prototxt lr_policy "step": base_lr * gamma^floor(iter / stepsize).  The power is a repeated product, so that the
// host and the device agree to the bit (the count is 0..2 over the solver's 400000 iterations).
VPK_TRAIN_FN float learning_rate(float base_lr, float gamma, int64_t stepsize, int64_t iter) {
    int64_t n = stepsize > 0 ? iter / stepsize : 0;
    float lr = base_lr;
    for (; n > 0 && lr != 0.0f; --n) lr *= gamma;
    return lr;
}

// Caffe's SGD update of one element (sgd_solver: Regularize "L2", ComputeUpdateValue, Blob::Update):
//   V <- mu V + lr_local (g + decay_local w);   w <- w - V
// lr_local = lr * lr_mult and decay_local = weight_decay * decay_mult (train_val.prototxt: 1, 1 for weights; 2, 0 for biases)
VPK_TRAIN_FN void sgd_update(float& w, float& v, float g, float lr_local, float decay_local, float mu) {
    const float vn = mu * v + lr_local * (g + decay_local * w);
    v = vn;
    w = w - vn;
}

// ---- dropout masks ------------------------------------------------------------------------------------------------------
// A counter-based hash: the keep bit of unit j of image b of a layer at an iteration is a pure function of
// (seed, iteration, layer, b, j) and of nothing else -- not of the launch geometry, nor of the other units.
//   h0 = mix(seed + GOLDEN * (iteration + 1))
//   h1 = mix(h0 ^ (layer << 32 | b))
//   h2 = mix(h1 ^ j)
// with mix = the finaliser of splitmix64 (Steele, Lea, Flood 2014) and GOLDEN = 0x9E3779B97F4A7C15.  The unit is kept when
// the top 24 bits of h2 are >= floor(p 2^24), p the dropout ratio: P(keep) = 1 - p to 2^-24.  layer: 6 (drop6) or 7 (drop7).
// The training set's draws (trainset_device.hpp) are the same hash under two more `layer` words: 0x41, the augmentation's
// uniform draw k of batch slot b, u_k = (mix(mask_key(seed, iteration, 0x41, b) ^ k) >> 11) 2^-53 in [0, 1), and 0x53, the
// sort key mix(mask_key(seed, epoch, 0x53, 0) ^ i) of example i in an epoch's shuffled order.
VPK_TRAIN_FN uint64_t mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

VPK_TRAIN_FN uint64_t mask_key(uint64_t seed, uint64_t iteration, uint32_t layer, uint32_t b) {
    const uint64_t h0 = mix64(seed + 0x9E3779B97F4A7C15ull * (iteration + 1ull));
    return mix64(h0 ^ (((uint64_t)layer << 32) | (uint64_t)b));
}

VPK_TRAIN_FN uint32_t mask_threshold(float dropout_ratio) {
    const float p = dropout_ratio < 0.0f ? 0.0f : (dropout_ratio > 1.0f ? 1.0f : dropout_ratio);
    return (uint32_t)(p * 16777216.0f);
}

VPK_TRAIN_FN uint8_t mask_bit(uint64_t key, uint32_t j, uint32_t threshold) {
    return (uint32_t)(mix64(key ^ (uint64_t)j) >> 40) >= threshold ? 1 : 0;
}

}  // namespace vpk_train

#endif
