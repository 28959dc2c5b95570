// train_store.hpp -- the parameters of a trainer: float32 master weights and their momentum as one list of blobs (weight,
// bias, weight, bias, ... in layer order), with the solver's numbers and the iteration.  vpk_train_state holds one with six
// blobs, vpk_convtrain_state one with two per CONV layer; the load / store / momentum / iteration entry points of both units
// are these functions under the unit's own name.
#ifndef VPK_TRAIN_STORE_HPP_
#define VPK_TRAIN_STORE_HPP_

#include "vpk_internal.hpp"

#pragma GCC visibility push(hidden)   // host helpers of two units of one library: nothing here is an export

struct vpk_param_store {
    static constexpr int MAX_BLOBS = 64;
    int n = 0;                        // blobs
    size_t count[MAX_BLOBS] = {};     // elements of every blob
    float* w[MAX_BLOBS] = {};         // the blobs on the device
    float* v[MAX_BLOBS] = {};         // ... and their momentum
    vpk_train_params p = {};
    long long iteration = 0;
    bool loaded = false;              // vpk_*_load has run: the weights mean something

    // allocates every blob and its momentum, stopping at the first failure (free() takes back what exists)
    hipError_t alloc(const size_t* counts, int blobs) {
        n = blobs;
        hipError_t e = hipSuccess;
        for (int i = 0; i < n && e == hipSuccess; ++i) {
            count[i] = counts[i];
            e = hipMalloc((void**)&w[i], count[i] * 4);
            if (e == hipSuccess) e = hipMalloc((void**)&v[i], count[i] * 4);
        }
        return e;
    }
    void free() {
        for (int i = 0; i < n; ++i) {
            if (w[i]) (void)hipFree(w[i]);
            if (v[i]) (void)hipFree(v[i]);
            w[i] = v[i] = nullptr;
        }
    }
};

// Weights or momentum between the host's blobs and the device, after the stream's work.  s: the trainer's store, null when
// the handle has none.  `who` names the entry point in every message.  The two units differ in where a null `blobs` is
// looked at: the head (silent_null) answers VPK_ERR_ARG without a message and before it asks for a trainer; the stack
// answers after, with a message, and only when it has blobs to name.
inline int vpk_store_copy(vpk_handle* h, vpk_param_store* s, const char* who, void* const* blobs, bool momentum, bool to_device,
                          bool need_loaded, bool silent_null) {
    if (!h) return VPK_ERR_ARG;
    const std::string name(who);
    if (s && need_loaded && !s->loaded) return vpk_fail(h, VPK_ERR_STATE, (name + " before the trainer's load").c_str());
    if (silent_null && !blobs) return VPK_ERR_ARG;
    if (!s) return vpk_fail(h, VPK_ERR_STATE, (name + ": the handle has no such trainer").c_str());
    for (int i = 0; i < s->n; ++i)
        if (!blobs || !blobs[i]) return vpk_fail(h, VPK_ERR_ARG, (name + ": a blob is null").c_str());
    VPK_HIP(h, hipSetDevice(h->device));
    VPK_HIP(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < s->n; ++i) {
        float* dev = momentum ? s->v[i] : s->w[i];
        if (to_device) VPK_HIP(h, hipMemcpy(dev, blobs[i], s->count[i] * 4, hipMemcpyHostToDevice));
        else VPK_HIP(h, hipMemcpy(blobs[i], dev, s->count[i] * 4, hipMemcpyDeviceToHost));
    }
    return VPK_OK;
}

// the weights of a solver started from a caffemodel: zero momentum, iteration 0
inline int vpk_store_load(vpk_handle* h, vpk_param_store* s, const char* who, const void* const* blobs, bool silent_null) {
    if (const int rc = vpk_store_copy(h, s, who, (void* const*)blobs, false, true, false, silent_null)) return rc;
    for (int i = 0; i < s->n; ++i) VPK_HIP(h, hipMemsetAsync(s->v[i], 0, s->count[i] * 4, h->stream));
    VPK_HIP(h, hipStreamSynchronize(h->stream));
    s->iteration = 0;
    s->loaded = true;
    return VPK_OK;
}

inline int vpk_store_set_iteration(vpk_handle* h, vpk_param_store* s, const char* who, long long iteration) {
    if (!h) return VPK_ERR_ARG;
    const std::string name(who);
    if (!s) return vpk_fail(h, VPK_ERR_STATE, (name + ": the handle has no such trainer").c_str());
    if (iteration < 0) return vpk_fail(h, VPK_ERR_ARG, (name + ": iteration < 0").c_str());
    s->iteration = iteration;
    return VPK_OK;
}

inline int vpk_store_get_iteration(const vpk_param_store* s, long long* iteration_out) {
    if (!s || !iteration_out) return VPK_ERR_ARG;
    *iteration_out = s->iteration;
    return VPK_OK;
}

#pragma GCC visibility pop

#endif
