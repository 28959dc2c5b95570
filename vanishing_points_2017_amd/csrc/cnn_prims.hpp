// cnn_prims.hpp -- what the CNN's matrix-core kernels share below their schedules: the vector types, the counted wait and the
// LDS-only barrier, LDS-DMA, and the persistent tile queue.  Included by vpk_cnn.hip FIRST and at file scope (it includes
// wave_prims.hpp and so the HIP runtime: it must not be opened for the first time inside the namespace vpk_cnn.hip nests the
// later kernel headers in); every cnn_*.hpp names it for its types, its include guard makes that a no-op.  Everything here is a
// typedef or force-inlined, so it adds no symbol and moves none.
//
// WHY THESE OPERATIONS ARE INLINE ASM.  hipcc keeps its own count of the vector-memory operations it has emitted and puts an
// s_waitcnt in front of the first use of what they load.  Three things follow, and whoever touches a kernel of this unit has to know them:
//   * The compiler must not see them.  It knows that the global_load_lds builtin writes LDS and puts `s_waitcnt vmcnt(0)` in front of the
//     next ds_read -- which drains the stage that was just issued and defeats the pipeline; with operations in between that it cannot
//     count it falls back to vmcnt(0) as well.  An asm statement is outside its bookkeeping, so completion is counted by hand:
//     wait_vmcnt<N>() = at most N vector-memory operations of this wave still outstanding; they retire in order.  What one wave has
//     waited for is published to the others by a barrier.
//   * The s_nop pads.  hipcc may have written an asm statement's SGPR operands with v_readlane / v_readfirstlane right before it, and
//     its hazard recogniser does not look inside the statement: VALU-writes-SGPR -> VMEM needs 5 wait states.  The two s_mov and the
//     `s_nop 2` in front of a DMA load give them, the `s_nop 4` in front of the queue's atomic likewise.
//   * M0 carries the wave-uniform LDS byte address of a DMA's destination (the hardware adds lane * size).  It is compiler-reserved, so
//     it is saved and restored inside the statement.
// The 16-byte DMA, the wait and the one-string barrier are wave_prims.hpp's (the EM smoother uses them too): one assembly string per
// instruction in the library.
#ifndef VPK_CNN_PRIMS_HPP_
#define VPK_CNN_PRIMS_HPP_

#include "wave_prims.hpp"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));      // the accumulator of a 32 x 32 matrix instruction
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));      // the A / B operand of a K16 (K32) bf16 matrix instruction
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- waits and barriers ----
// at most N vector-memory operations of this wave still outstanding
template <int N>
__device__ __forceinline__ void wait_vmcnt() { vpk::wait_vm<N>(); }
// workgroup barrier that orders LDS traffic only: global loads and stores stay in flight across it (__syncthreads also waits
// for vmcnt(0), i.e. one HBM round trip).  Two statements: the compiler may schedule between the wait and the barrier;
// raw_barrier() is the same pair as one string, which it may not.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}
using vpk::raw_barrier;

// ---- LDS-DMA: the 64 lanes of a wave move 16 (4) bytes each from (sbase + voff), sbase wave-uniform, to LDS at lds_dst + 16 (4) * lane:
//      no staging registers, no ds_write ----
using vpk::lds_addr_of;
using vpk::lds_dma16;
// the 4-byte form: the f32 GEMM's im2col panel is a gather, one element per lane
__device__ __forceinline__ void lds_dma4(unsigned voff, const void* sbase, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 2\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// ---- the persistent tile queue ----
// Persistent workgroups over a dynamic queue of tiles (work items): the first gridDim.x are taken statically (tile = blockIdx.x),
// the rest from the layer's atomic counter.  (With a static grid the workgroups are dealt round-robin to the XCDs, and CUs
// that another stream's kernel holds -- the EM runs beside the CNN -- make their XCD the straggler.)  The next index is fetched
// at the start of a tile and handed to the workgroup through LDS, so its latency is hidden.  Two slots used in turn: with one,
// thread 0 of a wave that has gone round could overwrite the index before a slower wave has read it -- no barrier separates
// that read from the next write.
//     __shared__ int s_next[2];
//     TileQueue queue{s_next};
//     for (int tile = blockIdx.x; tile < total;) {
//         int nx = queue.request(counter);  ...issue...  wait;  asm volatile("" : "+v"(nx));  queue.publish(nx);  barrier;  ...
//         tile = queue.next();
//     }
// Two forms of the fetch; which one a kernel uses is part of its schedule:
//   * request + publish (hand-issued): thread 0 issues the returning atomic at the top of the tile as the OLDEST outstanding
//     vector-memory operation of its wave, so the kernel's first counted wait retires it.  The compiler does not know that the
//     asm's result register is still being loaded: the kernel pins it (the empty asm above; on its OWN variable -- pinned as a
//     parameter in here, conv_gemm_dma_kernel's fused variant compiles to other code) behind that wait, and publish() stands
//     between the pin and the barrier that follows the wait.
//   * take (immediate): the compiler's atomicAdd, waited for and stored at once by thread 0 -- for kernels whose tile starts
//     with global loads of the compiler's own, which would wait for the atomic anyway.  At least one barrier must separate it
//     from the next() / peek() that reads the slot.
// The members are all of it for the f32 GEMM, the triples GEMM, the two dense and the two Winograd kernels.  The conv1 kernels
// run further ahead (conv1_direct_kernel two tiles, conv1_pieces_kernel an item that spans several tiles) and choose their slots
// themselves: take(counter, slot) and peek(slot), and their mid-loop fetch stays their own statement.  conv_pieces_kernel writes
// the same protocol out (its comment says why).
struct TileQueue {
    int* s_next;            // the kernel's __shared__ int[2]
    int parity = 0;

    // -> the register the atomic's result will land in (thread 0's; 0 elsewhere): not to be read before the pin
    __device__ __forceinline__ int request(int* counter) {
        int nx = 0;
        if (threadIdx.x == 0)    // ONE lane (s_nop 4, sc0 = returning: see the header comment)
            asm volatile("s_nop 4\n\tglobal_atomic_add %0, %1, %2, %3 sc0" : "=v"(nx) : "v"(0), "v"(1), "s"(counter) : "memory");
        return nx;
    }
    __device__ __forceinline__ void publish(int nx) {
        if (threadIdx.x == 0) s_next[parity] = nx + (int)gridDim.x;
    }
    __device__ __forceinline__ void take(int* counter, int slot) {
        if (threadIdx.x == 0) s_next[slot] = atomicAdd(counter, 1) + (int)gridDim.x;
    }
    __device__ __forceinline__ void take(int* counter) { take(counter, parity); }
    __device__ __forceinline__ int peek(int slot) const { return __builtin_amdgcn_readfirstlane(s_next[slot]); }
    __device__ __forceinline__ int next() {
        const int t = peek(parity);
        parity ^= 1;
        return t;
    }
};

}  // namespace
#endif
