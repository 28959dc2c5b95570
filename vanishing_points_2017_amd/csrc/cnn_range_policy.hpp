// cnn_range_policy.hpp -- RECOMPUTE_EXACT: compact a chunk's flagged images, run the exact configuration over them under a
// device count, scatter their maps back.  Included by vpk_cnn.hip after run_forward.
#ifndef VPK_CNN_RANGE_POLICY_HPP_
#define VPK_CNN_RANGE_POLICY_HPP_

namespace {

// ---- range policy RECOMPUTE_EXACT (vpk_cnn_set_range_policy) ----------------------------------------------------------------------
// After the pair pass of a chunk, on the handle's stream and with no host wait:
//   1. range_compact_kernel: the chunk's per-image words -> list[0] = count of flagged images, list[1 ..] their indices in order;
//   2. range_gather_kernel: their rasters -> slots 0 .. count - 1 of the arena's fp32-input region (R_IN: the exact configuration's conv1
//      reads rasters itself and never touches it);
//   3. the forward of vpk_cnn_set_algorithm(2) with the default conv1 over those slots.  The host does not know the count: every kernel
//      is launched for the whole chunk and reads list[0] (FwdCtl::live) -- the persistent ones size their tile queue by it, the others
//      exit at once for slots at or beyond it; with nothing flagged every launch is empty.  It is the same computation as that forward
//      run on the flagged rasters as one batch, so the maps are the same bits;
//   4. range_scatter_kernel: the maps (in fc6's output region, dead once fc7 has read it) -> their rows of `out`.
// The pair pass's activations are dead by then: the pass reuses the arena, no extra workspace.
__global__ __launch_bounds__(1024) void range_compact_kernel(const unsigned* __restrict__ img_range, int nb, int* __restrict__ list,
                                                             unsigned long long* __restrict__ recomputed) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int i0 = 0; i0 < nb; i0 += 1024) {
        const int i = i0 + tid;
        const bool f = i < nb && img_range[i] != 0u;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(f);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = base, all = 0;
        for (int w = 0; w < 16; ++w) {
            off += w < wave ? wsum[w] : 0;
            all += wsum[w];
        }
        if (f) list[1 + off + __popcll(m & ((1ull << lane) - 1ull))] = i;
        base += all;
        __syncthreads();                                 // (wsum is rewritten by the next round)
    }
    if (tid == 0) {
        list[0] = base;
        if (base) atomicAdd(recomputed, (unsigned long long)base);
    }
}

// slot s < list[0]: the raster of image list[1 + s] (250 000 bytes = 62 500 words: the rasters are 4-byte aligned; 8 workgroups per slot;
// Px = float: the float image, 250 000 words -- the size of an image's R_IN)
template <typename Px>
__global__ __launch_bounds__(256) void range_gather_kernel(const Px* __restrict__ sphere, const int* __restrict__ list,
                                                           Px* __restrict__ slots) {
    constexpr int WORDS = 250000 * (int)sizeof(Px) / 4;
    const int s = blockIdx.y;
    if (s >= list[0]) return;
    const unsigned* src = reinterpret_cast<const unsigned*>(sphere + (size_t)list[1 + s] * 250000);
    unsigned* dst = reinterpret_cast<unsigned*>(slots + (size_t)s * 250000);
    for (int q = blockIdx.x * 256 + threadIdx.x; q < WORDS; q += gridDim.x * 256) dst[q] = src[q];
}

// slot s < list[0]: its 400-float map -> row list[1 + s] of out
__global__ __launch_bounds__(128) void range_scatter_kernel(const float* __restrict__ maps, const int* __restrict__ list,
                                                            float* __restrict__ out) {
    const int s = blockIdx.x;
    if (s >= list[0]) return;
    const float* src = maps + (size_t)s * 400;
    float* dst = out + (size_t)list[1 + s] * 400;
    for (int q = threadIdx.x; q < 400; q += 128) dst[q] = src[q];
}

// the exact recompute of a chunk's flagged images (nb <= MAX_CHUNK; the arena holds nb images: the pair pass ran just before)
int recompute_flagged(vpk_handle* h, Images img, int nb, float* out, const unsigned* img_range) {
    vpk_cnn_state* S = h->cnn;
    hipStream_t st = h->stream;
    size_t off_fca = 0;
    for (int i = 0; i < R_FCA; ++i) off_fca += (size_t)S->act_batch * REGION_FLOATS[i];
    void* slots = S->act.p;                                                 // R_IN (region 0): 4 bytes per raster byte (one float image) of room
    float* maps = S->act.p + off_fca;                                       // R_FCA: 4096 floats per image of room
    hipLaunchKernelGGL(range_compact_kernel, dim3(1), dim3(1024), 0, st, img_range, nb, S->rc_list.p, S->rc_total.p);
    if (img.f32)
        hipLaunchKernelGGL(range_gather_kernel<float>, dim3(8, (unsigned)nb), dim3(256), 0, st, img.f(), S->rc_list.p, static_cast<float*>(slots));
    else
        hipLaunchKernelGGL(range_gather_kernel<uint8_t>, dim3(8, (unsigned)nb), dim3(256), 0, st, img.u8(), S->rc_list.p, static_cast<uint8_t*>(slots));
    CnnConfig exact = S->cfg;                    // exact operands, every kernel reads the device count (cnn_plan.hpp)
    exact.algorithm = 2; exact.fusion = 3; exact.precision = 0; exact.profiling = false;
    const int rc = run_forward(h, exact, Images{slots, img.f32}, nb, maps, -1, nullptr, FwdCtl{S->range_word.p + 1, nullptr, S->rc_list.p});
    if (rc) return rc;
    hipLaunchKernelGGL(range_scatter_kernel, dim3((unsigned)nb), dim3(128), 0, st, maps, S->rc_list.p, out);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // namespace
#endif
