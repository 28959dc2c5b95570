// vpk_em.hip -- EM kernels and their C-ABI entry points (see include/vpk.h): the batch kernel with its time-slice
// session, and the fine-grained single-workgroup entry points, whose bodies are em_hooks.hpp's.
//
// Compiled with -ffp-contract=off (see em_device.hpp).  One persistent workgroup of EM_THREADS
// threads per slot; workgroups pull images from a device-side queue (largest N first), so a
// ragged batch keeps every CU busy without host round trips.  What vpk_em_batch decides on the host before it
// launches -- the rules, slots and workgroups, the session's refusals, the header and session layouts -- is em_plan.hpp's.
#include "em_hooks.hpp"
#include "em_plan.hpp"
#include "vpk_internal.hpp"

using namespace vpk;

namespace {

// One workgroup per CU: the (non-inlined) phase functions touch ~250 VGPRs each -- the calling
// convention's callee-saved registers are striped through the file, so the allocator spreads over all of
// it -- and two waves per SIMD fill the register file.  Declaring the kernels for 1024 threads makes
// hipcc give the phases 128 VGPRs and two workgroups fit, but measured (r1): every phase slows down by
// 15-40 % (spills, narrower smoother) and the batch gains nothing at YUD sizes, +5 % at the stress shape.
constexpr int EM_BOUND = EM_THREADS;
#define VPK_SHARED_DECL Shared& sh = SH()

struct EmBatchArgs {
    int B;
    const long long* offsets;   // device, B+1
    const int* order;           // device, B (image indices, largest first)
    int* queue;                 // device counter
    double* l;
    const double* lp;
    const float* cnn;
    const unsigned char* sphere;
    int ssize;
    const double* init_vp;
    int n_init;
    vpk_em_params prm;
    EmLayout L;
    double* scratch;
    int max_vp;
    double* vp_out;
    double* sigma_out;
    double* counts_out;
    double* counts_w_out;
    int* num_vp_out;
    long long* assoc_out;
    int* iterations_out;
    int* status_out;
    unsigned* flags_out;
    double* metric_out;
    double* trace_out;
    int wt_doubles;
    int smoother;               // vpk_em_set_smoother
    vpk_em_dist_out dist;       // all null = not requested
};

// ---- time-sliced launches (vpk_em_set_time_slice) ------------------------------------------------
// An image that is not finished when its launch's deadline passes is parked as an EmCarry entry: the next
// launch on the handle drains the entries of the previous one before it takes fresh images.  Entries of
// images that were never started (the deadline passed first) carry slot = -1.
struct EmCarry {
    EmCtx c;
    EmOut o;
    int iter;     // -1: not started; >= 0: resume at the top of this iteration (state in the slot)
    int slot;     // -1: none yet
};
// Two lists per launch: images that have been STARTED (they own a slot) and images that have not.  A launch
// drains the started list before it touches anything else, which bounds the slots in use: every started entry
// is taken by a workgroup right at the beginning of the launch, so before the deadline each workgroup holds
// exactly one image, a new image starts only on a free workgroup, and after the deadline nothing starts --
// at most one started image per workgroup is ever parked (S_k <= workgroups for every launch k, by induction),
// and a free workgroup always finds a free slot among 2 x workgroups + 8.
struct EmSliceArgs {
    int enabled;
    long long budget_ticks;   // 0 = no deadline (flush): everything runs to completion
    int* ctr;                 // started: [0] consumed, [1] count of `in`, [2] appended to `out`; unstarted: [3], [4], [5]
    EmCarry* in_started;
    EmCarry* out_started;
    EmCarry* in_waiting;
    EmCarry* out_waiting;
    int cap_started, cap_waiting;
    int* busy;                // slot flags
    int nslots;
};

// take a free slot (session mode: slots outlive the launch, so they are not tied to the workgroup).  The invariant
// below (EmSliceArgs) guarantees a free slot; should it ever be broken the search gives up after a bounded number of
// sweeps (slots are released by images that FINISH, so a short sleep between sweeps is all that helps) and returns -1:
// the image is reported with VPK_EM_NO_SLOT instead of hanging the GPU.
constexpr int EM_SLOT_SWEEPS = 1 << 16;
VPK_DEV int acquire_slot(const EmSliceArgs& ss) {
    Shared& sh = SH();
    if (tid() == 0) {
        int got = -1;
        const int start = (block_id() * 2) % ss.nslots;
        for (int sweep = 0; sweep < EM_SLOT_SWEEPS && got < 0; ++sweep) {
            for (int k = 0; k < ss.nslots && got < 0; ++k) {
                const int s = (start + k) % ss.nslots;
                if (atomicCAS(&ss.busy[s], 0, 1) == 0) got = s;
            }
            if (got < 0) __builtin_amdgcn_s_sleep(127);
        }
        sh.ibuf[7] = got;
    }
    block_sync();
    const int slot = sh.ibuf[7];
    block_sync();
    return slot;
}

// pop the next entry of a parked list (workgroup-uniform result; -1 = exhausted)
VPK_DEV int pop_entry(int* head, const int* count) {
    Shared& sh = SH();
    if (tid() == 0) {
        int e = -1;
        const int n = *count;
        if (n > 0) { e = atomicAdd(head, 1); if (e >= n) e = -1; }
        sh.ibuf[7] = e;
    }
    block_sync();
    const int e = sh.ibuf[7];
    block_sync();
    return e;
}

// One instantiation per distance measure of the EM (em_run.hpp): the measure is a compile-time parameter, never a branch.
template <int MEASURE>
__global__ __launch_bounds__(EM_BOUND) void em_batch_kernel(EmBatchArgs a, EmSliceArgs ss) {
    VPK_SHARED_DECL;
    const long long t_start = clock_ticks();
    const long long deadline = (ss.enabled && ss.budget_ticks > 0) ? t_start + ss.budget_ticks : EM_NO_DEADLINE;
    bool started_left = ss.enabled != 0, waiting_left = ss.enabled != 0;
    for (;;) {
        EmCtx c;
        EmOut o;
        EmSlice sl;
        sl.deadline = deadline;
        sl.start_iter = -1;
        int slot = -1;
        bool have = false;
        // 1. images suspended by the previous launch (they own their slots), 2. images it could not start
        if (started_left) {
            const int e = pop_entry(&ss.ctr[0], &ss.ctr[1]);
            if (e >= 0) {
                const EmCarry& k = ss.in_started[e];
                c = k.c; o = k.o; sl.start_iter = k.iter; slot = k.slot;
                have = true;
            } else {
                started_left = false;
            }
        }
        if (!have && waiting_left) {
            const int e = pop_entry(&ss.ctr[3], &ss.ctr[4]);
            if (e >= 0) {
                const EmCarry& k = ss.in_waiting[e];
                c = k.c; o = k.o;
                have = true;
            } else {
                waiting_left = false;
            }
        }
        // 3. fresh images of this call
        if (!have) {
            if (tid() == 0) sh.ibuf[7] = atomicAdd(a.queue, 1);
            block_sync();
            const int q = sh.ibuf[7];
            block_sync();
            if (q >= a.B) break;
            const int img = a.order[q];
            const long long off = a.offsets[img];
            c.N = (int)(a.offsets[img + 1] - off);
            c.l = (gdp)(a.l + 3 * off);
            c.lp = (cgdp)(a.lp + 4 * off);
            c.cnn = (cgfp)(a.cnn + (size_t)img * NCELL);
            c.sphere = (cgbp)(a.sphere + (size_t)img * a.ssize * a.ssize);
            c.ssize = a.ssize;
            c.init_vp = a.init_vp ? (cgdp)(a.init_vp + (size_t)img * a.n_init * 3) : (cgdp) nullptr;
            c.n_init = a.n_init;
            c.prm = a.prm;
            c.wt_doubles = a.wt_doubles;
            c.smoother = a.smoother;
            o.max_vp = a.max_vp;
            o.vp = a.vp_out + (size_t)img * a.max_vp * 3;
            o.sigma = a.sigma_out + (size_t)img * a.max_vp;
            o.counts = a.counts_out + (size_t)img * a.max_vp;
            o.counts_w = a.counts_w_out + (size_t)img * a.max_vp;
            o.num_vp = a.num_vp_out + img;
            o.assoc = a.assoc_out + off;
            o.iterations = a.iterations_out + img;
            o.status = a.status_out + img;
            o.flags = a.flags_out + img;
            o.metric = a.metric_out ? a.metric_out + (size_t)off * a.max_vp : nullptr;
            o.trace = a.trace_out ? a.trace_out + (size_t)img * (a.prm.num_iter + 1) * TRACE_COLS : nullptr;
            if (a.dist.p_v) {
                o.d_pv = a.dist.p_v + (size_t)img * a.max_vp;
                o.d_angles = a.dist.angles + (size_t)img * a.max_vp * 2;
                o.d_pl = a.dist.p_l + off;
                o.d_plv = a.dist.p_lv + (size_t)off * a.max_vp;
                o.d_pvl = a.dist.p_vl + (size_t)off * a.max_vp;
                o.d_lvsq = a.dist.lvsq + (size_t)off * a.max_vp;
            }
        }
        // An image that has not been started when the deadline has passed is parked as it is -- unless its
        // list is full: then it runs now, TO COMPLETION (a longer launch, never a lost image; with the launch's
        // deadline it would take a slot, suspend at its first checkpoint and the workgroup would start the next one:
        // more suspended images than workgroups, which is what the slot count rules out).
        bool park_unstarted = false;
        bool list_full = false;
        if (ss.enabled && slot < 0 && deadline != EM_NO_DEADLINE) {
            if (tid() == 0) {
                int e = -1;
                if (clock_ticks() >= deadline) {
                    e = atomicAdd(&ss.ctr[5], 1);
                    if (e >= ss.cap_waiting) e = -2;
                }
                sh.ibuf[7] = e;
            }
            block_sync();
            const int e = sh.ibuf[7];
            block_sync();
            list_full = e == -2;
            if (e >= 0) {
                if (tid() == 0) {
                    EmCarry& k = ss.out_waiting[e];
                    k.c = c; k.o = o; k.iter = -1; k.slot = -1;
                }
                park_unstarted = true;
            }
        }
        if (park_unstarted) continue;
        if (list_full) sl.deadline = EM_NO_DEADLINE;
        if (slot < 0) {
            slot = ss.enabled ? acquire_slot(ss) : block_id();
            if (slot < 0) {                    // bounded wait expired (see acquire_slot): report, do not hang
                if (tid() == 0) { *o.status = VPK_EM_NO_SLOT; *o.num_vp = 0; *o.iterations = 0; *o.flags = 0; }
                block_sync();
                continue;
            }
            bind_scratch(c, a.scratch + (size_t)slot * a.L.total_doubles, a.L, c.prm.do_split != 0);
        }
        int result = em_run<MEASURE>(c, o, sl);
        while (result == EM_SUSPENDED) {       // only with a deadline; at most one per workgroup and launch (see above)
            if (tid() == 0) {
                int e = atomicAdd(&ss.ctr[2], 1);
                if (e < ss.cap_started) {
                    EmCarry& k = ss.out_started[e];
                    k.c = c; k.o = o; k.iter = sl.start_iter; k.slot = slot;
                } else {
                    e = -1;                    // the list is full: this image is resumed right here and runs on
                }
                sh.ibuf[7] = e;
            }
            block_sync();
            const bool parked = sh.ibuf[7] >= 0;
            block_sync();
            if (parked) break;
            sl.deadline = EM_NO_DEADLINE;
            result = em_run<MEASURE>(c, o, sl);   // resumes from the state it has just saved in its slot
        }
        if (result == EM_SUSPENDED) {
        } else if (ss.enabled) {
            block_sync();
            if (tid() == 0) { __threadfence(); atomicExch(&ss.busy[slot], 0); }
        }
    }
}

// between two time-sliced launches: what the last launch parked becomes the next launch's input list
__global__ void em_rotate_kernel(int* ctr, int cap_waiting, int cap_started) {
    ctr[1] = ctr[2] < cap_started ? ctr[2] : cap_started;   // (the counters keep counting when a list is full)
    ctr[0] = 0;
    ctr[2] = 0;
    ctr[4] = ctr[5] < cap_waiting ? ctr[5] : cap_waiting;   // the counter keeps counting when the list is full
    ctr[3] = 0;
    ctr[5] = 0;
}

// ---- fine-grained kernels (one workgroup, unit parity) ------------------------------------------
// The bodies are em_hooks.hpp's, which the tests' host build compiles too; a kernel only makes the context: value-initialised,
// the launch's LDS budget and smoother, the scratch slot bound.
VPK_DEV EmCtx kernel_ctx(int wt_doubles, int smoother) {
    EmCtx c{};
    c.wt_doubles = wt_doubles; c.smoother = smoother;
    return c;
}
VPK_DEV EmCtx kernel_ctx(int wt_doubles, int smoother, double* ws, const EmLayout& L) {
    EmCtx c = kernel_ctx(wt_doubles, smoother);
    bind_scratch(c, ws, L, false);
    return c;
}

__global__ __launch_bounds__(EM_BOUND) void pairwise_kernel(int n, const double* lp, EmLayout L, double* ws,
                                                              double* lsim_out, double* lscore_out,
                                                              double* langle_out, int smoother) {
    EmCtx c = kernel_ctx(WT_DOUBLES, smoother, ws, L);
    hook_pairwise(c, n, lp, lsim_out, lscore_out, langle_out);
}

__global__ __launch_bounds__(EM_BOUND) void init_vps_kernel(const float* cnn, const unsigned char* sphere,
                                                              int ssize, int num_max, double* v0_out,
                                                              int* m0_out, float* weights_out) {
    EmCtx c = kernel_ctx(WT_DOUBLES, 0);
    hook_init_vps(c, cnn, sphere, ssize, num_max, v0_out, m0_out, weights_out);
}

__global__ __launch_bounds__(EM_BOUND) void estep_kernel(int n, int m, const double* lp, const float* cnn,
                                                           const double* v, double* s, EmLayout L, double* ws,
                                                           double* p_v_out, double* lvsq_out, double* p_vl_out,
                                                           double* p_l_out, int smoother) {
    EmCtx c = kernel_ctx(WT_DOUBLES, smoother, ws, L);
    hook_estep(c, n, m, lp, cnn, v, s, p_v_out, lvsq_out, p_vl_out, p_l_out);
}

__global__ __launch_bounds__(EM_BOUND) void weight_matrix_kernel(int n, int m, const double* p_vl,
                                                                   const double* lweight, const double* lsim,
                                                                   double bias, EmLayout L, double* ws,
                                                                   double* w_out, int smoother, int wt_doubles) {
    EmCtx c = kernel_ctx(wt_doubles, smoother, ws, L);
    hook_weight_matrix(c, n, m, p_vl, lweight, lsim, bias, w_out);
}

__global__ __launch_bounds__(EM_BOUND) void estep_smooth_kernel(int n, int m, const double* lp, const float* cnn,
                                                                  const double* v, double* s, const double* lweight,
                                                                  const double* lsim, double bias, EmLayout L, double* ws,
                                                                  double* p_vl_out, double* w_out, int* info_out,
                                                                  int smoother, int wt_doubles) {
    EmCtx c = kernel_ctx(wt_doubles, smoother, ws, L);
    hook_estep_smooth(c, n, m, lp, cnn, v, s, lweight, lsim, bias, p_vl_out, w_out, info_out);
}

__global__ __launch_bounds__(EM_BOUND) void mstep_kernel(int n, int m, const double* l, const double* w,
                                                           EmLayout L, double* ws, double* vp_out,
                                                           int* valid_out) {
    EmCtx c = kernel_ctx(WT_DOUBLES, 0, ws, L);
    hook_mstep(c, n, m, l, w, vp_out, valid_out);
}

__global__ __launch_bounds__(EM_BOUND) void mstep_full_kernel(int n, int m, const double* l, const double* w,
                                                                const double* lvsq, const double* p_vl, const int* assoc,
                                                                const double* cur, double max_stdd, double s_thresh,
                                                                EmLayout L, double* ws, double* vp_out, double* s_out,
                                                                double* err_out, int* removed_out, int smoother) {
    EmCtx c = kernel_ctx(WT_DOUBLES, smoother, ws, L);
    hook_mstep_full(c, n, m, l, w, lvsq, p_vl, assoc, cur, max_stdd, s_thresh, vp_out, s_out, err_out, removed_out);
}

__global__ __launch_bounds__(EM_BOUND) void line_counts_kernel(int n, int m, const double* lp, const double* v,
                                                                 const double* s, const double* w, const double* lweight,
                                                                 double thresh, EmLayout L, double* ws, double* counts_out,
                                                                 double* counts_w_out, long long* assoc_out) {
    EmCtx c = kernel_ctx(WT_DOUBLES, 0, ws, L);
    hook_line_counts(c, n, m, lp, v, s, w, lweight, thresh, counts_out, counts_w_out, assoc_out);
}

__global__ __launch_bounds__(EM_BOUND) void cluster2_kernel(int n, double* D, int* member, int* csize,
                                                              int* labels_out, unsigned* flags_out, int smoother, int wt_doubles) {
    hook_cluster2(n, D, member, csize, labels_out, flags_out, smoother, wt_doubles);
}

int em_prepare(vpk_handle* h) {
    if (h->em_ready) return VPK_OK;
    for (auto kernel : {(const void*)em_batch_kernel<VPK_DIST_ANGLE>, (const void*)em_batch_kernel<VPK_DIST_DOTPROD>,
                        (const void*)pairwise_kernel, (const void*)init_vps_kernel, (const void*)estep_kernel,
                        (const void*)weight_matrix_kernel, (const void*)estep_smooth_kernel, (const void*)mstep_kernel,
                        (const void*)mstep_full_kernel, (const void*)cluster2_kernel, (const void*)line_counts_kernel})
        VPK_HIP(h, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)EM_LDS_BYTES_BIG));
    h->em_ready = true;
    return VPK_OK;
}

// What every fine-grained entry point does before its launch: the device, the kernels' LDS attribute and ws_bytes of
// h->small_ws (0: none) ...
int hook_begin(vpk_handle* h, size_t ws_bytes) {
    VPK_HIP(h, hipSetDevice(h->device));
    if (int rc = em_prepare(h)) return rc;
    return ws_bytes ? vpk_reserve(h, &h->small_ws, &h->small_ws_bytes, ws_bytes, "hipMalloc(workspace)") : VPK_OK;
}
// ... and the launch itself: one workgroup on the handle's stream
template <typename... P, typename... A>
int hook_launch(vpk_handle* h, void (*kernel)(P...), size_t lds_bytes, A... args) {
    hipLaunchKernelGGL(kernel, dim3(1), dim3(EM_THREADS), lds_bytes, h->stream, args...);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

// what the launch plan (em_plan.hpp) reads of the handle
EmFacts em_facts(const vpk_handle* h) {
    return EmFacts{h->cu_share, h->em_max_workgroups, h->total_mem, h->em_lds_doubles, h->em_slice_ms, h->em_slice_nmax,
                   h->em_started_cap, h->em_wait_cap, h->em_sess != nullptr, h->em_sess_slot_bytes, h->em_sess_slots,
                   h->em_sess_wgs, h->em_sess_layout, h->em_unflushed, h->em_ws_bytes};
}

// The previous launch's output lists become this launch's input lists.  List capacities: vpk_handle::em_wait_cap (images
// parked before they were started; a full list makes further ones run on) and ::em_started_cap (suspended images: at most
// one per workgroup, vpk_em_set_workgroups <= CUs)
EmSliceArgs sess_next(vpk_handle* h, double slice_ms) {
    const EmSessLayout v = em_sess_layout(h->em_sess_slots, h->em_started_cap, h->em_wait_cap, sizeof(EmCarry));
    char* base = (char*)h->em_sess;
    EmSliceArgs ss;
    ss.ctr = (int*)(base + v.head);
    hipLaunchKernelGGL(em_rotate_kernel, dim3(1), dim3(1), 0, h->stream, ss.ctr, h->em_wait_cap, h->em_started_cap);
    h->em_sess_in ^= 1;
    ss.enabled = 1;
    ss.budget_ticks = em_slice_ticks(slice_ms);
    ss.in_started = (EmCarry*)(base + v.started[h->em_sess_in]); ss.out_started = (EmCarry*)(base + v.started[h->em_sess_in ^ 1]);
    ss.in_waiting = (EmCarry*)(base + v.waiting[h->em_sess_in]); ss.out_waiting = (EmCarry*)(base + v.waiting[h->em_sess_in ^ 1]);
    ss.cap_started = h->em_started_cap; ss.cap_waiting = h->em_wait_cap;
    ss.busy = (int*)(base + v.busy); ss.nslots = h->em_sess_slots;
    return ss;
}

// the batch kernel of the handle's distance measure (vpk_em_set_distance_measure)
int em_launch(vpk_handle* h, int wgs, size_t lds_bytes, const EmBatchArgs& a, const EmSliceArgs& ss) {
    auto kernel = h->em_measure == VPK_DIST_DOTPROD ? em_batch_kernel<VPK_DIST_DOTPROD> : em_batch_kernel<VPK_DIST_ANGLE>;
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(EM_THREADS), lds_bytes, h->stream, a, ss);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

// launch that finishes every parked image (no deadline, no fresh images); asynchronous on the handle's stream
int em_flush(vpk_handle* h) {
    if (!h->em_unflushed) return VPK_OK;
    EmSliceArgs ss = sess_next(h, 0.0);
    EmBatchArgs a = {};
    a.B = 0;
    a.queue = ss.ctr + 8;                      // a counter that is never below B = 0
    a.L = h->em_sess_layout;
    a.scratch = (double*)h->em_ws;
    a.wt_doubles = h->em_sess_wt_doubles;
    a.smoother = h->em_smoother;
    if (int rc = em_launch(h, h->em_sess_wgs, h->em_sess_lds, a, ss)) return rc;   // (the measure that parked them: the setter refuses meanwhile)
    h->em_unflushed = false;
    return VPK_OK;
}

// the slot of a single-image call: m VPs, every array of the weighted EM, no split scratch
EmLayout small_layout(int n, int m) {
    return em_layout(n, (int)em_align((size_t)(m > 0 ? m : 1), 8), EM_WAVES, true, false);
}

// vpk_math_probe: the elementary functions exactly as this translation unit's kernels get them (same compiler flags, same
// ocml entry points as em_device.hpp's calls), one argument per thread.
__global__ void math_probe_kernel(int fn, long long n, const double* __restrict__ x, double* __restrict__ y) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double r;
    switch (fn) {
        case 0: r = exp(v); break;
        case 1: r = acos(v); break;
        case 2: r = asin(v); break;
        case 3: r = atan(v); break;
        case 4: r = sqrt(v); break;
        case 5: r = sin(v); break;
        case 6: r = cos(v); break;
        default: r = log(v); break;
    }
    y[i] = r;
}
}  // namespace

extern "C" {

int vpk_math_probe(vpk_handle* h, int fn, long long n, const double* x, double* y) {
    if (!h || fn < 0 || fn > 7 || n < 1 || !x || !y) return vpk_fail(h, VPK_ERR_ARG, "vpk_math_probe: bad argument");
    VPK_HIP(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, fn, n, x, y);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

int vpk_em_set_smoother(vpk_handle* h, int mode) {
    if (!h || mode < 0 || mode > 2) return vpk_fail(h, VPK_ERR_ARG, "vpk_em_set_smoother: mode must be 0, 1 or 2");
    h->em_smoother = mode;
    return VPK_OK;
}

int vpk_em_set_lds_panel(vpk_handle* h, int doubles) {
    if (!h || doubles < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_em_set_lds_panel: bad argument");
    if (h->em_unflushed) return vpk_fail(h, VPK_ERR_STATE, "vpk_em_set_lds_panel: images are parked: vpk_em_flush first");
    h->em_lds_doubles = doubles;
    return VPK_OK;
}

int vpk_em_set_distance_measure(vpk_handle* h, int measure) {
    if (!h) return VPK_ERR_ARG;
    if (measure != VPK_DIST_ANGLE && measure != VPK_DIST_DOTPROD)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_em_set_distance_measure: VPK_DIST_ANGLE or VPK_DIST_DOTPROD");
    if (h->em_unflushed)
        return vpk_fail(h, VPK_ERR_STATE, "vpk_em_set_distance_measure: images are parked: vpk_em_flush first");
    h->em_measure = measure;
    return VPK_OK;
}

int vpk_em_set_workgroups(vpk_handle* h, int max_workgroups) {
    if (!h || max_workgroups < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_em_set_workgroups: bad argument");
    h->em_max_workgroups = max_workgroups;
    return VPK_OK;
}

size_t vpk_em_workspace_bytes(const vpk_handle* h, int batch, int n_max, const vpk_em_params* p, int n_init) {
    if (!h || !p || batch < 1) return 0;
    return em_plan_slots(em_facts(h), batch, n_max, *p, n_init, n_init > 0, false).ws_bytes();
}

int vpk_em_batch(vpk_handle* h, int batch, const int64_t* offsets, double* l, const double* lp,
                 const float* cnn, const uint8_t* sphere, int sphere_size, const double* init_vp,
                 int n_init, const vpk_em_params* p, int max_vp, double* vp_out, double* sigma_out,
                 double* counts_out, double* counts_w_out, int32_t* num_vp_out, int64_t* assoc_out,
                 int32_t* iterations_out, int32_t* status_out, uint32_t* flags_out,
                 double* metric_out, double* trace_out) {
    if (!h) return VPK_ERR_ARG;
    const bool buffers = l && lp && cnn && sphere && vp_out && sigma_out && counts_out && counts_w_out && num_vp_out &&
                         assoc_out && iterations_out && status_out && flags_out;
    const EmPlan pl = em_plan(em_facts(h), batch, offsets, buffers, sphere_size, max_vp, p, n_init, init_vp != nullptr);
    if (pl.rule) {
        static const char* const what[] = {
            nullptr,
            "vpk_em_batch: null buffer or batch < 1",                                 // EM_PLAN_NULL
            "vpk_em_batch: bad sphere_size/max_vp",                                   // EM_PLAN_SPHERE
            "params is null",                                                         // EM_PLAN_PARAMS
            "num_iter out of range",                                                  // EM_PLAN_NUM_ITER
            "split_merge_freq < 1",                                                   // EM_PLAN_FREQ
            "num_init_vp must be 1..64",                                              // EM_PLAN_NUM_INIT
            "n_init must be 1..64",                                                   // EM_PLAN_N_INIT
            "vpk_em_batch: offsets not monotone",                                     // EM_PLAN_OFFSETS
            "vpk_em_batch: more than 46000 lines in one image",                       // EM_PLAN_LINES
            "vpk_em_batch: time-sliced slots exceed half of the device memory",       // EM_PLAN_SLICE_MEM
            "vpk_em_batch: the slot layout changed (more lines than vpk_em_set_time_slice was told, or other parameters) "
            "while images are parked: vpk_em_flush first",                            // EM_PLAN_SESS_CHANGED
            "vpk_em_batch: workspace would move while images are parked: vpk_em_flush first"};   // EM_PLAN_WS_MOVES
        static_assert(sizeof(what) / sizeof(what[0]) == EM_PLAN_WS_MOVES + 1, "one text per rule");
        return vpk_fail(h, em_rule_code(pl.rule), what[pl.rule]);
    }
    VPK_HIP(h, hipSetDevice(h->device));
    if (int rc = em_prepare(h)) return rc;
    if (!pl.sliced && h->em_unflushed) { if (int rc = em_flush(h)) return rc; }
    if (pl.new_session) {
        const size_t need = em_sess_layout(pl.slots, h->em_started_cap, h->em_wait_cap, sizeof(EmCarry)).total;
        if (int rc = vpk_reserve(h, &h->em_sess, &h->em_sess_bytes, need, "hipMalloc(EM session)")) return rc;
        VPK_HIP(h, hipMemsetAsync(h->em_sess, 0, need, h->stream));
        h->em_sess_slot_bytes = pl.slot_bytes; h->em_sess_slots = pl.slots; h->em_sess_wgs = pl.wgs;
        h->em_sess_layout = pl.L; h->em_sess_in = 0;
        h->em_sess_wt_doubles = pl.mode.wt_doubles; h->em_sess_lds = pl.mode.lds_bytes;
    }
    if (int rc = vpk_reserve(h, &h->em_ws, &h->em_ws_bytes, pl.ws_bytes(), "hipMalloc(EM workspace)")) return rc;
    // header: offsets | order, filled in the pinned staging; the queue counter behind them is zeroed on the device
    void* host;
    if (int rc = vpk_stage_begin(h, h->em_hdr, pl.staged_bytes(), &host)) return rc;
    memcpy(host, offsets, (size_t)(batch + 1) * sizeof(int64_t));
    em_order(batch, offsets, (int*)((char*)host + pl.off_bytes));
    if (int rc = vpk_stage_commit(h, h->em_hdr, pl.staged_bytes(), "hipMalloc(EM header)", 256)) return rc;
    char* hdr = (char*)h->em_hdr.dev;
    VPK_HIP(h, hipMemsetAsync(hdr + pl.staged_bytes(), 0, 256, h->stream));

    EmBatchArgs a;
    a.B = batch;
    a.offsets = (const long long*)hdr;
    a.order = (const int*)(hdr + pl.off_bytes);
    a.queue = (int*)(hdr + pl.staged_bytes());
    a.l = l; a.lp = lp; a.cnn = cnn; a.sphere = sphere; a.ssize = sphere_size;
    a.init_vp = init_vp; a.n_init = n_init;
    a.prm = *p;
    a.L = pl.L;
    a.scratch = (double*)h->em_ws;
    a.max_vp = max_vp;
    a.vp_out = vp_out; a.sigma_out = sigma_out; a.counts_out = counts_out; a.counts_w_out = counts_w_out;
    a.num_vp_out = num_vp_out; a.assoc_out = (long long*)assoc_out; a.iterations_out = iterations_out;
    a.status_out = status_out; a.flags_out = flags_out; a.metric_out = metric_out; a.trace_out = trace_out;
    a.dist = vpk_em_dist_out{};
    if (h->em_dist_set) {                  // consumed by this call
        a.dist = h->em_dist;
        h->em_dist_set = false;
    }
    a.wt_doubles = pl.mode.wt_doubles;
    a.smoother = h->em_smoother;
    EmSliceArgs ss = {};
    if (pl.sliced) {
        ss = sess_next(h, h->em_slice_ms);
        h->em_unflushed = true;
    }
    return em_launch(h, pl.wgs, pl.mode.lds_bytes, a, ss);
}

int vpk_em_set_distribution_out(vpk_handle* h, const vpk_em_dist_out* d) {
    if (!h) return VPK_ERR_ARG;
    if (!d) { h->em_dist_set = false; return VPK_OK; }
    if (!d->p_v || !d->angles || !d->p_l || !d->p_lv || !d->p_vl || !d->lvsq)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_em_set_distribution_out: every buffer must be given");
    if (h->em_slice_ms > 0.0)
        return vpk_fail(h, VPK_ERR_STATE, "vpk_em_set_distribution_out: not available with time-sliced launches");
    h->em_dist = *d;
    h->em_dist_set = true;
    return VPK_OK;
}

int vpk_em_set_time_slice(vpk_handle* h, double slice_ms, int n_max) {
    if (!h || !(slice_ms >= 0.0) || n_max < 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_em_set_time_slice: bad argument");
    VPK_HIP(h, hipSetDevice(h->device));
    { int rc0 = em_prepare(h); if (rc0) return rc0; }
    if (slice_ms == 0.0 && h->em_unflushed) { int rc = em_flush(h); if (rc) return rc; }
    h->em_slice_ms = slice_ms;
    h->em_slice_nmax = n_max;
    return VPK_OK;
}

int vpk_em_flush(vpk_handle* h) {
    if (!h) return VPK_ERR_ARG;
    VPK_HIP(h, hipSetDevice(h->device));
    return em_flush(h);
}

int vpk_pairwise(vpk_handle* h, int n, const double* lp, double* lsim_out, double* lscore_out,
                 double* langle_out) {
    if (!h || n < 1 || !lp || !lsim_out || !lscore_out || !langle_out) return vpk_fail(h, VPK_ERR_ARG, "vpk_pairwise: bad argument");
    const EmLayout L = small_layout(n, 8);
    if (int rc = hook_begin(h, L.total_doubles * 8)) return rc;
    return hook_launch(h, pairwise_kernel, EM_LDS_BYTES, n, lp, L, (double*)h->small_ws, lsim_out, lscore_out, langle_out,
                       h->em_smoother);
}

int vpk_init_vps(vpk_handle* h, const float* cnn, const uint8_t* sphere, int sphere_size, int num_max,
                 double* v0_out, int32_t* m0_out, float* weights_out) {
    if (!h || !cnn || !sphere || !v0_out || !m0_out || !weights_out || num_max < 1 || num_max > MAXM ||
        sphere_size < GRIDN)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_init_vps: bad argument");
    if (int rc = hook_begin(h, 0)) return rc;
    return hook_launch(h, init_vps_kernel, EM_LDS_BYTES, cnn, sphere, sphere_size, num_max, v0_out, (int*)m0_out, weights_out);
}

int vpk_estep(vpk_handle* h, int n, int m, const double* lp, const float* cnn, const double* v, double* s,
              double* p_v_out, double* lvsq_out, double* p_vl_out, double* p_l_out) {
    if (!h || n < 1 || m < 1 || m > MAXM || !lp || !cnn || !v || !s || !p_v_out || !lvsq_out || !p_vl_out || !p_l_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_estep: bad argument");
    const EmLayout L = small_layout(n, m);
    if (int rc = hook_begin(h, L.total_doubles * 8)) return rc;
    return hook_launch(h, estep_kernel, EM_LDS_BYTES, n, m, lp, cnn, v, s, L, (double*)h->small_ws, p_v_out, lvsq_out,
                       p_vl_out, p_l_out, h->em_smoother);
}

int vpk_weight_matrix(vpk_handle* h, int n, int m, const double* p_vl, const double* lweight,
                      const double* lsim, double bias, double* w_out) {
    if (!h || n < 1 || m < 1 || m > MAXM || !p_vl || !lweight || !lsim || !w_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_weight_matrix: bad argument");
    const EmLayout L = small_layout(n, m);
    if (int rc = hook_begin(h, L.total_doubles * 8)) return rc;
    // the batch kernel's LDS budget, so that this entry point takes the same smoother an image of this size takes there
    const EmMode mode = em_mode(h->em_lds_doubles);
    return hook_launch(h, weight_matrix_kernel, mode.lds_bytes, n, m, p_vl, lweight, lsim, bias, L, (double*)h->small_ws,
                       w_out, h->em_smoother, mode.wt_doubles);
}

int vpk_estep_smooth(vpk_handle* h, int n, int m, const double* lp, const float* cnn, const double* v, double* s,
                     const double* lweight, const double* lsim, double bias, double* p_vl_out, double* w_out,
                     int32_t* info_out) {
    if (!h || n < 1 || m < 1 || m > MAXM || !lp || !cnn || !v || !s || !lweight || !lsim || !p_vl_out || !w_out || !info_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_estep_smooth: bad argument");
    const EmLayout L = small_layout(n, m);
    if (int rc = hook_begin(h, L.total_doubles * 8)) return rc;
    // the batch kernel's LDS budget (as vpk_weight_matrix): the E-step plans the panel and the smoother takes it as they do there
    const EmMode mode = em_mode(h->em_lds_doubles);
    return hook_launch(h, estep_smooth_kernel, mode.lds_bytes, n, m, lp, cnn, v, s, lweight, lsim, bias, L,
                       (double*)h->small_ws, p_vl_out, w_out, (int*)info_out, h->em_smoother, mode.wt_doubles);
}

int vpk_mstep(vpk_handle* h, int n, int m, const double* l, const double* w, double* vp_out, int32_t* valid_out) {
    if (!h || n < 1 || m < 1 || m > MAXM || !l || !w || !vp_out || !valid_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_mstep: bad argument");
    const EmLayout L = em_layout(n, (int)em_align((size_t)m, 8), EM_WAVES, false, false);
    if (int rc = hook_begin(h, L.total_doubles * 8)) return rc;
    return hook_launch(h, mstep_kernel, EM_LDS_BYTES, n, m, l, w, L, (double*)h->small_ws, vp_out, (int*)valid_out);
}

int vpk_mstep_full(vpk_handle* h, int n, int m, const double* l, const double* w, const double* lvsq, const double* p_vl,
                   const int32_t* assoc, const double* cur, double max_stdd, double s_thresh, double* vp_out,
                   double* s_out, double* err_out, int32_t* removed_out) {
    if (!h || n < 1 || m < 1 || m > MAXM || !l || !w || !lvsq || !p_vl || !cur || !vp_out || !s_out || !err_out || !removed_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_mstep_full: bad argument");
    const EmLayout L = em_layout(n, (int)em_align((size_t)m, 8), EM_WAVES, false, false);
    if (int rc = hook_begin(h, L.total_doubles * 8)) return rc;
    return hook_launch(h, mstep_full_kernel, EM_LDS_BYTES, n, m, l, w, lvsq, p_vl, (const int*)assoc, cur, max_stdd, s_thresh,
                       L, (double*)h->small_ws, vp_out, s_out, err_out, (int*)removed_out, h->em_smoother);
}

int vpk_line_counts(vpk_handle* h, int n, int m, const double* lp, const double* v, const double* s, const double* w,
                    const double* lweight, double thresh, double* counts_out, double* counts_w_out, int64_t* assoc_out) {
    if (!h || n < 1 || m < 1 || m > MAXM || !lp || !v || !s || !w || !lweight || !counts_out || !counts_w_out || !assoc_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_line_counts: bad argument");
    const EmLayout L = small_layout(n, m);
    if (int rc = hook_begin(h, L.total_doubles * 8)) return rc;
    return hook_launch(h, line_counts_kernel, EM_LDS_BYTES, n, m, lp, v, s, w, lweight, thresh, L, (double*)h->small_ws,
                       counts_out, counts_w_out, (long long*)assoc_out);
}

int vpk_cluster2(vpk_handle* h, int n, const double* ldist, int32_t* labels_out, uint32_t* flags_out) {
    if (!h || n < 3 || !ldist || !labels_out || !flags_out) return vpk_fail(h, VPK_ERR_ARG, "vpk_cluster2: bad argument");
    if (int rc = hook_begin(h, (size_t)n * n * 8 + (size_t)2 * n * 4 + 64)) return rc;
    double* D = (double*)h->small_ws;
    int* member = (int*)(D + (size_t)n * n);
    VPK_HIP(h, hipMemcpyAsync(D, ldist, (size_t)n * n * 8, hipMemcpyDeviceToDevice, h->stream));
    // the whole CU's LDS, as the batch kernel has it when it runs one workgroup per CU: sets of up to 126 lines cluster in LDS
    return hook_launch(h, cluster2_kernel, EM_LDS_BYTES_BIG, n, D, member, member + n, (int*)labels_out, (unsigned*)flags_out,
                       h->em_smoother, WT_DOUBLES_BIG);
}

}  // extern "C"
