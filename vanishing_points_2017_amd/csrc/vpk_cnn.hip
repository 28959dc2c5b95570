// vpk_cnn.hip -- AlexNet-500 forward (cnn/deploy.prototxt:1-304) as hand-written gfx950 kernels.
//
// Caffe conventions reproduced: cross-correlation, OIHW weights, grouped
// convolution splits input/output channels contiguously, MAX pooling with CEIL output size and
// border-clipped windows, LRN across channels x * (1 + alpha/n * sum x^2)^-beta, InnerProduct
// weight (out,in) over the C*H*W-flattened input, Dropout = identity at TEST, input = uint8
// raster minus the mean blob with no scaling (evaluation.py:34-38).
//
// All arithmetic is fp32 ("parity mode"): the convolutions and the fully connected layers run as
// implicit GEMMs on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32, 157 TF dense peak),
// tiles staged through LDS (k-major, conflict-free fragment reads), global->register prefetch of
// tile t+1 issued before the MFMAs of tile t, bias + ReLU fused in the epilogue.  Weights are
// re-packed once at load time into k-major [K][M] panels so every staging load is a coalesced
// 16-byte access.  Activations live in HBM for the whole batch (B x 96 x 123 x 123 fp32 is
// 0.6 GB at B = 102; 288 GB of HBM3E makes chunking unnecessary up to B ~ 4000).
#include "vpk_internal.hpp"

#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BK = 16;          // K depth of one LDS stage
constexpr int CONV_THREADS = 256;

struct ConvDims {
    int B, IC, Hp, Wp;          // input: IC = channels per group; Hp x Wp = PADDED plane (zero border = conv padding)
    int OC, OH, OW;             // output (OC = channels per group)
    int groups;
    int K;                      // IC*KH*KW (unpadded)
    int Kp;                     // K padded to a multiple of BK
    int Mp;                     // OC padded to a multiple of BM
    int N;                      // B*OH*OW
    int ksplit;                 // split-K factor (dense layers); 1 = fused epilogue
    int relu;
    int OHp, OWp, opad;         // output plane layout: (oh, ow) is stored at (oh + opad, ow + opad) of an OHp x OWp plane
};

// --------------------------------------------------------------------------------------------
// implicit-GEMM convolution / dense layer
//   C[m][n] = sum_k Wp[k][m] * X[k][n],  m = output channel, n = (b, oh, ow), k = (ic, kh, kw)
// WAVES_M x WAVES_N waves, each owning TM x TN MFMA tiles of 32 x 32.
// --------------------------------------------------------------------------------------------
// LDS-DMA implicit GEMM (every conv / dense layer; for conv1 only the unfused / tapped paths -- its input is then
// pre-converted to fp32 phase planes by prep_input_kernel; the default conv1 is conv1_direct_kernel below):
// both operand tiles go HBM -> LDS with global_load_lds (no staging VGPRs, no ds_write), three LDS
// stages, raw s_barrier + counted s_waitcnt vmcnt(N) so that the DMA of stage t+2 stays in flight
// across the barrier that publishes stage t+1 (cdna_hip_programming.md T3/T4).  The weights panel is
// lane-linear 16-byte pieces; the im2col panel is one 4-byte gather per lane, lanes = 64 consecutive
// output positions of one k row, so the LDS image Bs[k][n] is lane-linear too.
//
// Addressing costs no vector instructions inside the K loop: activations are stored in planes that
// already carry the convolution's zero border (the producer writes the interior, the border is zeroed
// when the workspace is allocated), so every tap of every output position is an in-range load and
// address = (scalar: tile base + table[k]) + (per-lane constant: position of the patch origin).  The
// DMA uses the saddr form (64-bit SGPR base + 32-bit VGPR offset); the lane offsets are computed once
// per workgroup.  Columns beyond N (last tile) re-read column N-1 and are not stored.
// --------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_ptr_t;

template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// LDS-DMA issued from inline asm: hipcc knows that the global_load_lds builtin writes LDS and puts an
// s_waitcnt vmcnt(0) in front of the next ds_read, which drains the stage that was just issued and
// defeats the pipeline.  An asm statement is outside its bookkeeping; completion is counted by hand
// (wait_stage below).  M0 = wave-uniform LDS byte address of the destination (the hardware adds
// lane * size); M0 is compiler-reserved, so it is saved and restored inside the statement.  The three
// scalar instructions in front of the load give 5 wait states: hipcc may have written the SGPR operands
// with v_readlane / v_readfirstlane just before (VALU-writes-SGPR -> VMEM hazard it cannot see in asm).
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(lds_ptr_t)p; }
__device__ __forceinline__ void dma16(unsigned voff, const void* sbase, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 2\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void dma4(unsigned voff, const void* sbase, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 2\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// conv1 + norm1 + pool1 as ONE kernel (C1FUSE): a tile's 128 columns are a 2-D patch of 7 x 17 conv1 outputs
// (all 96 channels: one M tile, so the LRN across channels is local to the tile); after the K loop the patch
// goes to LDS (over the then idle stage buffers), is normalised in place and max-pooled to 3 x 8 outputs per
// channel, and only those are written -- conv1's 0.59 GB output (B = 102) never exists.  Neighbouring patches
// share one conv row / column (pooling windows overlap by one), i.e. 7/6 x 17/16 = 1.24x the MFMA work.
constexpr int C1_PR = 7, C1_PC = 17;               // conv outputs per patch (rows x cols): 119 of the tile's 128 columns
constexpr int C1_QR = 3, C1_QC = 8;                // pooled outputs per patch
constexpr int C1_OUT = 123, C1_POOL = 61;          // conv1 / pool1 output size (deploy.prototxt:9-55)
constexpr int C1_TR = (C1_POOL + C1_QR - 1) / C1_QR, C1_TC = (C1_POOL + C1_QC - 1) / C1_QC;   // 21 x 8 patches per image
constexpr int C1_LD = 129;                         // row stride of the patch in LDS ([channel][column])
constexpr int C1_PH = 4, C1_PW = 125;              // conv1 reads its input as 4 x 4 stride-4 phase planes of 125 x 125 (prep_input_kernel)

template <int WAVES_M, int WAVES_N, int TM, int TN, bool DENSE, bool C1FUSE = false, int NST = 3, int WPC = 3>
__global__ __launch_bounds__(CONV_THREADS, WPC) void conv_gemm_dma_kernel(ConvDims d, const float* __restrict__ in,
                                                                     const float* __restrict__ wp,
                                                                     const float* __restrict__ bias,
                                                                     const unsigned* __restrict__ ktab,
                                                                     float* __restrict__ out, int stride,
                                                                     int* __restrict__ tile_counter, int total_tiles,
                                                                     const int* __restrict__ live) {
    constexpr int BM = WAVES_M * TM * 32;
    constexpr int BN = WAVES_N * TN * 32;
    static_assert(BN == 128, "the B-tile loader assumes 128 columns");
    static_assert(!C1FUSE || (BM == 96 && TN == 1 && !DENSE), "the fused conv1 tile is 96 channels x 128 columns");
    static_assert(NST == 2 || NST == 3, "two or three LDS stages");
    constexpr int STAGE_FLOATS = NST * BK * (BM + BN);
    constexpr int LDS_FLOATS = C1FUSE ? (96 * C1_LD > STAGE_FLOATS ? 96 * C1_LD : STAGE_FLOATS) : STAGE_FLOATS;
    __shared__ __attribute__((aligned(16))) float lds_raw[LDS_FLOATS];
    float (*As)[BK][BM] = reinterpret_cast<float (*)[BK][BM]>(lds_raw);
    float (*Bs)[BK][BN] = reinterpret_cast<float (*)[BK][BN]>(lds_raw + NST * BK * BM);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    // Persistent workgroups over a dynamic tile queue: the first gridDim.x tiles are taken statically, the
    // rest from an atomic counter.  (With a static grid the workgroups are dealt round-robin to the XCDs, and
    // CUs that another stream's kernel holds -- the EM runs beside the CNN -- make their XCD the straggler.)
    // The next index is fetched at the start of a tile and published through LDS, so its latency is hidden.
    __shared__ int s_next[2];
    int parity = 0;
    if (!C1FUSE && live) {                              // recompute pass (vpk_cnn_set_range_policy): the device count's images only
        d.B = __builtin_amdgcn_readfirstlane(*live);
        d.N = d.B * d.OH * d.OW;
        total_tiles = d.groups * d.ksplit * ((d.N + BN - 1) / BN) * (d.Mp / BM);
    }
    for (int tile = blockIdx.x; tile < total_tiles;) {
    int nx = 0;
    if (tid == 0)    // ONE lane; the oldest outstanding vector-memory op of wave 0: complete at the first wait_stage
        // (s_nop 4: hipcc may have produced the SGPR pair with v_readlane right before this statement and
        //  cannot see that the instruction inside reads it -- VALU-writes-SGPR -> VMEM needs 5 wait states)
        asm volatile("s_nop 4\n\tglobal_atomic_add %0, %1, %2, %3 sc0" : "=v"(nx) : "v"(0), "v"(1), "s"(tile_counter) : "memory");
    const int mtiles = d.Mp / BM;
    int bid = tile;
    const int mt = bid % mtiles; bid /= mtiles;
    const int ntiles = (d.N + BN - 1) / BN;
    const int nt = bid % ntiles; bid /= ntiles;
    const int ks = bid % d.ksplit;
    const int g = bid / d.ksplit;
    const int ksteps_total = d.Kp / BK;
    const int ksteps_per = (ksteps_total + d.ksplit - 1) / d.ksplit;
    const int kt0 = ks * ksteps_per;
    const int kt1 = (kt0 + ksteps_per) < ksteps_total ? (kt0 + ksteps_per) : ksteps_total;
    const float* wpan = wp + (size_t)g * d.Kp * d.Mp + (size_t)mt * BM;

    // ---- per-lane constants of the B (im2col / dense) gather -------------------------------------
    const int kset = wave >> 1;                       // waves 0,1 -> k 0..7 ; waves 2,3 -> k 8..15
    const int ohw = d.OH * d.OW;
    int n = nt * BN + (tid & 127);
    n = n < d.N ? n : d.N - 1;                        // tail columns re-read the last valid one
    const float* bbase;                               // wave-uniform base of this tile's gather
    unsigned boff;                                    // this lane's byte offset from it
    if (C1FUSE) {
        // tile = (image, patch row, patch column); column j of the tile = conv output (6 pr + j / 17, 16 pc + j % 17),
        // clamped into the blob (overhanging positions only ever meet pooling windows that Caffe clips away)
        const int pc = tile % C1_TC, pr = (tile / C1_TC) % C1_TR, b = tile / (C1_TC * C1_TR);
        const int j = tid & 127;
        int oh = (C1_PR - 1) * pr + j / C1_PC, ow = (C1_PC - 1) * pc + j % C1_PC;
        oh = oh < C1_OUT ? oh : C1_OUT - 1;
        ow = ow < C1_OUT ? ow : C1_OUT - 1;
        bbase = in + (size_t)b * d.IC * d.Hp * d.Wp;
        boff = (unsigned)(oh * d.Wp + ow) * 4u;
    } else if (DENSE) {
        // dense layers: the activation rows are K-contiguous, so the B tile is fetched as 16-byte pieces ALONG K --
        // one piece = 4 consecutive k of one column; a DMA instruction = one k-quad x 64 consecutive columns.  (4-byte
        // pieces, one k row x 64 columns per instruction, touch 64 cache lines for 256 bytes: the texture-address
        // path then takes as long as the stage's MFMAs.)  The tile lands in LDS as [k quad][column][4].
        bbase = in;
        int nd = nt * BN + (wave & 1) * 64 + lane;
        nd = nd < d.N ? nd : d.N - 1;
        boff = (unsigned)nd * (unsigned)d.K * 4u;
    } else {
        const int b_first = (nt * BN) / ohw;          // first image of the tile (scalar)
        const int b = n / ohw;
        const int r = n - b * ohw;
        const int oh = r / d.OW, ow = r - oh * d.OW;
        const int plane = d.Hp * d.Wp;
        bbase = in + ((size_t)b_first * d.groups + g) * d.IC * plane;
        boff = (unsigned)((b - b_first) * d.groups * d.IC * plane + oh * stride * d.Wp + ow * stride) * 4u;
    }
    // ---- per-lane constants of the A (weights) pieces --------------------------------------------
    constexpr int A_F4 = (BK * BM) / 4;
    constexpr int A_IT = (A_F4 + CONV_THREADS - 1) / CONV_THREADS;
    unsigned aoff[A_IT];
#pragma unroll
    for (int r = 0; r < A_IT; ++r) {
        const int idx = r * CONV_THREADS + wave * 64 + lane;
        const int kk = (idx * 4) / BM, m = (idx * 4) % BM;
        aoff[r] = (unsigned)(kk * d.Mp + m) * 4u;
    }
    const unsigned as_base = lds_addr(&As[0][0][0]), bs_base = lds_addr(&Bs[0][0][0]);
    auto issue = [&](int kt, int buf) {
        const int k0 = kt * BK;
        const float* abase = wpan + (size_t)k0 * d.Mp;
#pragma unroll
        for (int r = 0; r < A_IT; ++r) {
            const int idx0 = r * CONV_THREADS + wave * 64;         // wave-uniform first float4 of this piece
            if (idx0 < A_F4)
                dma16(aoff[r], abase, __builtin_amdgcn_readfirstlane(as_base + (unsigned)((buf * BK * BM + idx0 * 4) * 4)));
        }
        if (DENSE) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {                            // this wave's two k quads (of four), its half of the columns
                const int kq = (wave >> 1) * 2 + q;
                dma16(boff, bbase + k0 + 4 * kq, __builtin_amdgcn_readfirstlane(
                          bs_base + (unsigned)((buf * BK * BN + (kq * BN + (wave & 1) * 64) * 4) * 4)));
            }
            return;
        }
        const int kb = k0 + kset * 8;
        unsigned e[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) e[q] = ktab[kb + q];            // wave-uniform byte offsets: scalar loads
#pragma unroll
        for (int q = 0; q < 8; ++q)
            dma4(boff, (const char*)bbase + e[q], __builtin_amdgcn_readfirstlane(
                                bs_base + (unsigned)(((buf * BK + kset * 8 + q) * BN + (wave & 1) * 64) * 4)));
    };
    // DMA instructions one thread issues per stage (waves whose A piece falls outside issue one less)
    constexpr int A_FULL = A_F4 / CONV_THREADS;                    // pieces every wave issues
    constexpr bool A_PARTIAL = (A_F4 % CONV_THREADS) != 0;         // extra piece for the first waves only
    auto wait_stage = [&](bool keep_one_in_flight) {
        // wait until only the newest stage's DMA (if any) is still outstanding for this wave
        const bool extra = A_PARTIAL && (A_FULL * CONV_THREADS + wave * 64 < A_F4);
        constexpr int B_PER = DENSE ? 2 : 8;                       // B-tile DMA instructions per thread and stage
        if (!keep_one_in_flight) wait_vmcnt<0>();
        else if (extra) wait_vmcnt<A_FULL + 1 + B_PER>();
        else wait_vmcnt<A_FULL + B_PER>();
    };

    const int arow = wm * TM * 32 + (lane & 31);
    const int bcol = wn * TN * 32 + (lane & 31);
    const int khalf = lane >> 5;
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = kt1 - kt0;
    constexpr int AHEAD = NST - 1;                      // stages in flight ahead of the one being multiplied
    if (nk > 0) issue(kt0, 0);
    if (AHEAD > 1 && nk > 1) issue(kt0 + 1, 1);
    wait_stage(AHEAD > 1 && nk > 1);
    asm volatile("" : "+v"(nx));                        // the atomic's result has landed (it is older than stage 0)
    if (tid == 0) s_next[parity] = nx + (int)gridDim.x;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int t = 0; t < nk; ++t) {
        const int buf = t % NST;
        if (t + AHEAD < nk) issue(kt0 + t + AHEAD, (t + AHEAD) % NST);
        // operands of k step k2 + 2 are requested before the MFMAs of step k2 are issued (left to itself the compiler
        // puts each step's LDS reads right in front of their use: one exposed LDS round trip per step and wave)
        float af[2][TM], bf[2][TN];
        auto operands = [&](int k2) {
            const int o = (k2 >> 1) & 1;
#pragma unroll
            for (int i = 0; i < TM; ++i) af[o][i] = As[buf][k2 + khalf][arow + i * 32];
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bf[o][j] = DENSE ? (&Bs[buf][0][0])[(((k2 + khalf) >> 2) * BN + bcol + j * 32) * 4 + ((k2 + khalf) & 3)]
                                 : Bs[buf][k2 + khalf][bcol + j * 32];
        };
        operands(0);
#pragma unroll
        for (int k2 = 0; k2 < BK; k2 += 2) {
            if (k2 + 2 < BK) operands(k2 + 2);
            __builtin_amdgcn_sched_barrier(0);
            const int o = (k2 >> 1) & 1;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[o][i], bf[o][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        wait_stage(AHEAD > 1 && t + 2 < nk);            // stage t+1 has landed (own pieces) ...
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                   // ... for every wave; stage t's buffer is free again
    }

    // Epilogue.  The 32 x 32 accumulator tile holds rows 8q + 4 khalf + (0..3) in registers 4q .. 4q + 3: a
    // group of eight rows (one q) is in or out of range as a whole (OC is a multiple of 8 in every layer),
    // its bias is eight consecutive floats fetched by ONE scalar load, and a lane's addresses are a 64-bit
    // base (its column) plus 32-bit row offsets.  (Per-element vector bias loads were each followed by
    // s_waitcnt vmcnt(0), which also waits for the store just issued: 48-64 store round trips in series per
    // tile, more than half of conv1's tile time.)
    if (C1FUSE) {
        // ---- fused epilogue: bias + ReLU -> LDS patch -> LRN (in place) -> 3x3/2 max pool -> store ----
        float (*Cs)[C1_LD] = reinterpret_cast<float (*)[C1_LD]>(lds_raw);    // [channel][column]; the stage buffers are idle now
        const int pc = tile % C1_TC, pr = (tile / C1_TC) % C1_TR, b = tile / (C1_TC * C1_TR);
        const int col = wn * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m0 = __builtin_amdgcn_readfirstlane(i * 32 + 8 * q);
                const float* bp = bias + m0;                        // wave-uniform: scalar load of 8 floats
                float bl[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) bl[e] = bp[e];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = acc[i][0][4 * q + e] + (khalf ? bl[4 + e] : bl[e]);
                    Cs[m0 + 4 * khalf + e][col] = v > 0.f ? v : 0.f;
                }
            }
        __syncthreads();
        {   // LRN across channels (deploy.prototxt:34-44): two threads per column, 48 channels each, 5-deep window
            const int p = tid & 127, c0 = (tid >> 7) * 48;
            float v0 = c0 >= 2 ? Cs[c0 - 2][p] : 0.f, v1 = c0 >= 1 ? Cs[c0 - 1][p] : 0.f;
            float v2 = Cs[c0][p], v3 = Cs[c0 + 1][p];
            const float e0 = c0 + 48 < 96 ? Cs[c0 + 48][p] : 0.f, e1 = c0 + 49 < 96 ? Cs[c0 + 49][p] : 0.f;
            __syncthreads();                                        // every raw halo value has been read
            const float an = 1e-4f / 5.f;
#pragma unroll 8
            for (int k = 0; k < 48; ++k) {
                const float v4 = k + 2 < 48 ? Cs[c0 + k + 2][p] : (k + 2 == 48 ? e0 : e1);
                const float sc = 1.f + an * (v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3 + v4 * v4);
                const float r = __builtin_amdgcn_rsqf(sc);
                Cs[c0 + k][p] = v2 * (r * __builtin_amdgcn_sqrtf(r));   // sc^-0.75
                v0 = v1; v1 = v2; v2 = v3; v3 = v4;
            }
        }
        __syncthreads();
        for (int e = tid; e < 96 * C1_QR * C1_QC; e += CONV_THREADS) {
            const int k = e / (C1_QR * C1_QC), o = e - k * (C1_QR * C1_QC);
            const int py = o / C1_QC, px = o - py * C1_QC;
            const int ph = C1_QR * pr + py, pw = C1_QC * pc + px;
            if (ph >= C1_POOL || pw >= C1_POOL) continue;
            float m = -3.402823466e38f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int r = 2 * py + dy, q = 2 * px + dx;
                    if ((C1_PR - 1) * pr + r < C1_OUT && (C1_PC - 1) * pc + q < C1_OUT) {   // Caffe clips the window
                        const float v = Cs[k][r * C1_PC + q];
                        m = v > m ? v : m;
                    }
                }
            out[((size_t)b * 96 + k) * d.OHp * d.OWp + (size_t)(ph + d.opad) * d.OWp + pw + d.opad] = m;
        }
        __syncthreads();                                            // the next tile's DMA overwrites the patch
    } else {
    const int oplane = d.OHp * d.OWp;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nn = nt * BN + wn * TN * 32 + j * 32 + (lane & 31);
        if (nn >= d.N) continue;
        const int bb = nn / ohw;
        const int rr = nn - bb * ohw;
        const int oh = rr / d.OW, ow = rr - oh * d.OW;
        if (d.ksplit == 1) {
            float* ocol = out + ((size_t)bb * d.groups + g) * d.OC * oplane + (size_t)(oh + d.opad) * d.OWp + ow + d.opad;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int m0 = __builtin_amdgcn_readfirstlane(mt * BM + wm * TM * 32 + i * 32 + 8 * q);
                    if (m0 >= d.OC) continue;                       // whole group of eight rows is padding
                    const float* bp = bias + g * d.OC + m0;         // wave-uniform: scalar load of 8 floats
                    float bl[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) bl[e] = bp[e];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v = acc[i][j][4 * q + e] + (khalf ? bl[4 + e] : bl[e]);
                        if (d.relu) v = v > 0.f ? v : 0.f;
                        ocol[(m0 + 4 * khalf + e) * oplane] = v;
                    }
                }
            }
        } else {
            float* prow = out + ((size_t)ks * d.N + nn) * d.OC;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int m0 = __builtin_amdgcn_readfirstlane(mt * BM + wm * TM * 32 + i * 32 + 8 * q);
                    if (m0 >= d.OC) continue;
#pragma unroll
                    for (int e = 0; e < 4; ++e) prow[m0 + 4 * khalf + e] = acc[i][j][4 * q + e];
                }
            }
        }
    }
    }
    tile = __builtin_amdgcn_readfirstlane(s_next[parity]);
    parity ^= 1;
    }   // tile loop
}

// --------------------------------------------------------------------------------------------
// conv1 + relu1 + norm1 + pool1 (deploy.prototxt:9-55) as a DIRECT convolution, one 512-thread workgroup per CU.
//
// conv1 is the odd layer: K = 121 only, so an implicit-GEMM tile spends more time on its im2col gather (256 LDS-DMA
// instructions per tile), prologue and epilogue than on its 8 K stages (measured: matrix pipes 42 % busy).  Here
//   * the whole weight panel (128 x 96, k-major) stays in LDS for the lifetime of the persistent workgroup,
//   * a tile = a 7 x 17 patch of conv outputs (all 96 channels); its RAW input patch (16 stride-4 phase planes x 9 x 19
//     pixels, 11 KB -- against 64 KB of im2col panel) is prefetched into registers under the previous tile's MFMAs,
//   * the B operand is read straight out of the raw patch: address = (patch position of the lane's column) + (offset of
//     tap k), the 32 tap offsets a lane needs live in registers,
//   * 8 waves x 16 columns, v_mfma_f32_16x16x4_f32, 6 M tiles per wave (24 accumulator registers),
//   * epilogue out of LDS: bias + ReLU -> patch [channel][column] -> LRN across channels in place -> 3x3/2 max pool
//     (windows clipped like Caffe) -> 3 x 8 pooled outputs per channel, written with conv2's border.
// Neighbouring patches share one conv row / column (1.24x the MFMA work); conv1's 0.59 GB blob (B = 102) never exists.
// --------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const f32x2 lds_cf32x2;
typedef __attribute__((address_space(3))) const float lds_cfloat;
constexpr int C1D_THREADS = 512;
constexpr int C1D_ALD = 96;                           // row stride of the weight panel in LDS: the four k rows a wave reads
                                                      // at once (k = 4s + lane/16) fall into disjoint bank quarters
constexpr int C1D_PY = 9, C1D_PX = 19, C1D_PXL = 20;  // rows / columns of one phase of the raw patch; LDS row stride
constexpr int C1D_XS = 16 * C1D_PY * C1D_PXL;         // floats per patch buffer
constexpr int C1D_KS = 31;                            // K steps of 4 taps: 121 taps -> 124 (rows 121..127 of the packed panel are 0)
constexpr int C1D_LD = 132;                           // row stride of the output patch [channel][column]: the four row groups
                                                      // a wave writes at once (rows 4 apart) hit disjoint bank quarters

// workgroup barrier that orders LDS traffic only: the pooled outputs' global stores stay in flight across it
// (__syncthreads also waits for vmcnt(0), i.e. one HBM write round trip per tile)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

#ifdef C1D_TIME
__device__ long long c1d_dbg[256 * 8 * 8];
#define C1D_T(i) { const long long t_ = (long long)__builtin_amdgcn_s_memtime(); tacc[i] += t_ - tprev; tprev = t_; }
#else
#define C1D_T(i)
#endif
// Px = float: the images of vpk_cnn_forward_f32 (Caffe's float32 blob before the mean), four pixels = one 16-byte word
template <typename Px = unsigned char>
__global__ __launch_bounds__(C1D_THREADS, 2) void conv1_direct_kernel(const Px* __restrict__ sphere,
                                                                      const float* __restrict__ mean, const float* __restrict__ wp,
                                                                      const float* __restrict__ bias, float* __restrict__ out,
                                                                      int OHp, int OWp, int opad, int* __restrict__ tile_counter,
                                                                      int total_tiles) {
    __shared__ __attribute__((aligned(16))) float As[128 * C1D_ALD];
    __shared__ __attribute__((aligned(16))) float Xs[C1D_XS];
    __shared__ __attribute__((aligned(16))) float Cs[96 + 4][C1D_LD];  // channel c in row c + 2; rows 0, 1, 98, 99 stay 0 (LRN halo)
    __shared__ int s_next[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c16 = lane & 15;
    if (tid < C1D_LD) Cs[0][tid] = Cs[1][tid] = Cs[98][tid] = Cs[99][tid] = 0.f;
    for (int idx = tid; idx < 128 * 96; idx += C1D_THREADS) {            // global [Kp = 128][Mp = 96] -> LDS [k][m % 16][m / 16]
        const int k = idx / 96, m = idx - k * 96;
        As[k * C1D_ALD + (m & 15) * 6 + (m >> 4)] = wp[idx];
    }
    // A operands: in K step s2 this lane feeds row k = 4 s2 + g, channels 16 i + c16 (i = 0..5) = six consecutive floats,
    // read as three 8-byte words at compile-time offsets from three base registers.  (The bases are made opaque: the
    // compiler would otherwise fuse the reads into ds_read2 forms, whose 8-bit offsets need a new base register -- one
    // VALU add, which costs matrix-pipe time here -- in every step.)
    lds_cf32x2* a0 = (lds_cf32x2*)&As[g * C1D_ALD + c16 * 6];
    lds_cf32x2* a1 = a0 + 1;
    lds_cf32x2* a2 = a0 + 2;
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2));
    // B operands: this lane's column of the tile and the LDS address of tap k = 4 s2 + g for it
    int col = wave * 16 + c16;
    col = col < C1_PR * C1_PC ? col : C1_PR * C1_PC - 1;                 // columns 119..127 repeat the last position, unused
    const int colbase = (col / C1_PC) * C1D_PXL + col % C1_PC;
    lds_cfloat* kb[C1D_KS];
#pragma unroll
    for (int s2 = 0; s2 < C1D_KS; ++s2) {
        const int k = 4 * s2 + g;
        const int kh = k / 11, kw = k - kh * 11;
        kb[s2] = (lds_cfloat*)&Xs[colbase + (k < 121 ? (((kh & 3) * 4 + (kw & 3)) * C1D_PY + (kh >> 2)) * C1D_PXL + (kw >> 2)
                                                      : 0)];           // rows 121..127 of the panel are 0
    }
    f32x4 bl[6];                                                         // bias of the 24 channels this lane's accumulators hold:
#pragma unroll                                                           //  the C operand of a tile's first MFMAs
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) bl[i][r] = bias[16 * i + 4 * g + r];
    // The input is read where the caller left it: the uint8 rasters and the mean blob (row-major, as loaded);
    // evaluation.py:35's float(image) - mean happens on the way into LDS.  (A pre-pass used to write that difference as
    // fp32 phase planes: 102 MB out and in per batch.)  A thread fetches QUADS: the four horizontally adjacent pixels
    // (4 X .. 4 X + 3) of raster row 4 Y + py' are one 4-byte word of the raster and one 16-byte word of the mean, and
    // they are the elements (Y, X) of the four phase planes (py', 0..3) -- 684 quads per patch, two per thread.
    constexpr int QUADS = C1_PH * C1D_PY * C1D_PX;                                 // 684
    constexpr int PRE = (QUADS + C1D_THREADS - 1) / C1D_THREADS;                   // quads per thread (2)
    constexpr int PRE_LAST = QUADS - (PRE - 1) * C1D_THREADS;                      // threads that hold a second one
    constexpr bool F32 = std::is_same<Px, float>::value;
    typedef typename std::conditional<F32, f32x4, unsigned>::type Raw;         // a quad of pixels
    int qoff[PRE], pdst[PRE], pyx[PRE];
#pragma unroll
    for (int u = 0; u < PRE; ++u) {
        const int e = tid + u * C1D_THREADS;
        const int pq = e / (C1D_PY * C1D_PX), rem = e - pq * (C1D_PY * C1D_PX);    // pq = py' (row phase)
        const int py = rem / C1D_PX, px = rem - py * C1D_PX;
        qoff[u] = (C1_PH * py + pq) * 500 + C1_PH * px;                            // pixel offset from the patch's first pixel
        pdst[u] = ((pq * C1_PH) * C1D_PY + py) * C1D_PXL + px;                     // LDS index in phase plane (pq, 0)
        pyx[u] = (pq << 16) | (py << 8) | px;
    }
    auto patch_load = [&](int tile, f32x4 (&v)[PRE], Raw (&v8)[PRE]) {
        const int pc = tile % C1_TC, pr = (tile / C1_TC) % C1_TR, b = tile / (C1_TC * C1_TR);
        const int y0 = (C1_PR - 1) * pr, x0 = (C1_PC - 1) * pc;
        const Px* img = sphere + (size_t)b * 500 * 500;
        if (pr < C1_TR - 1 && pc < C1_TC - 1) {        // the patch lies inside the planes: scalar base + per-thread offset
            const int origin = (C1_PH * y0) * 500 + C1_PH * x0;
#pragma unroll
            for (int u = 0; u < PRE; ++u) {
                const bool on = u < PRE - 1 || tid < PRE_LAST;
                const int o = on ? origin + qoff[u] : origin;
                v[u] = *reinterpret_cast<const f32x4*>(mean + o);
                v8[u] = *reinterpret_cast<const Raw*>(img + o);
            }
        } else {
#pragma unroll
            for (int u = 0; u < PRE; ++u) {            // overhang is clamped (those taps only reach conv outputs that no
                const int y = y0 + ((pyx[u] >> 8) & 255), x = x0 + (pyx[u] & 255);   //  pooling window uses)
                const int pq = pyx[u] >> 16;
                const int yc = y < C1_PW ? y : C1_PW - 1, xc = x < C1_PW ? x : C1_PW - 1;
                const bool on = u < PRE - 1 || tid < PRE_LAST;
                const int o = on ? (C1_PH * yc + pq) * 500 + C1_PH * xc : 0;
                v[u] = *reinterpret_cast<const f32x4*>(mean + o);
                v8[u] = *reinterpret_cast<const Raw*>(img + o);
            }
        }
    };
    auto patch_store = [&](const f32x4 (&v)[PRE], const Raw (&v8)[PRE]) {
#pragma unroll
        for (int u = 0; u < PRE; ++u)
            if (u < PRE - 1 || tid < PRE_LAST) {
#pragma unroll
                for (int q = 0; q < C1_PH; ++q) {
                    if constexpr (F32) Xs[pdst[u] + q * (C1D_PY * C1D_PXL)] = v8[u][q] - v[u][q];
                    else Xs[pdst[u] + q * (C1D_PY * C1D_PXL)] = (float)((v8[u] >> (8 * q)) & 255u) - v[u][q];
                }
            }
    };
    // dynamic tile queue (CUs held by other streams' kernels make static shares uneven); the index of the tile after
    // next is fetched one tile ahead, so the atomic's round trip is never waited for
    int tile = blockIdx.x;
    f32x4 pre[PRE];
    Raw pre8[PRE];
    if (tile < total_tiles) { patch_load(tile, pre, pre8); patch_store(pre, pre8); }
    if (tid == 0) s_next[0] = atomicAdd(tile_counter, 1) + (int)gridDim.x;
    __syncthreads();
    int next = __builtin_amdgcn_readfirstlane(s_next[0]);
    // Software pipeline across tiles: the LRN and the pooling of tile i-1 are issued between the MFMA steps of tile i, so
    // that per tile only "accumulators -> Cs" and "Cs -> LRN inputs" stand alone between barriers.  f32 MFMAs run at the
    // packed-f32 vector rate and do NOT overlap with VALU work of either wave of the SIMD (measured: a phase costs the
    // MFMA cycles of both waves PLUS their VALU cycles), so the epilogue is written for instruction count: packed f32
    // math, v_max3 / v_med3, unconditional halo reads, bias as the accumulators' initial value.
    const int lp = tid & 127, lc0 = (tid >> 7) * 24;                 // LRN: this thread's column and its first channel
    const int pk = tid < 96 * C1_QR ? tid / C1_QR : 95, ppy = tid % C1_QR;   // pooling: (channel, pooled row of the patch)
    const float* pool_src = &Cs[pk + 2][2 * ppy * C1_PC];
    f32x2 raw2[14];                                                  // ReLU'd conv outputs of the PREVIOUS tile: 24 channels + halo
#pragma unroll
    for (int k = 0; k < 14; ++k) raw2[k] = f32x2{0.f, 0.f};
    int ptile = -1;                                                  // the tile whose epilogue is pending
    // LRN across channels (deploy.prototxt:34-44), in place: out = v * (1 + alpha / 5 * sum of the 5 squares)^-0.75
    f32x2 sqa, sqb;                                                  // rolling squares of raw[2j .. 2j+3] and their pair sums
    float psa, psb;
    auto lrn_squares = [&]() {
#pragma clang fp contract(off)
        sqa = raw2[0] * raw2[0]; psa = sqa[0] + sqa[1];
        sqb = raw2[1] * raw2[1]; psb = sqb[0] + sqb[1];
    };
    auto lrn_two = [&](int j) {                                      // channels lc0 + 2 j, lc0 + 2 j + 1 (window = raw[2j .. 2j+5])
#pragma clang fp contract(off)     // the same roundings in the main loop and in the drain copy of this code (a tile's bits must
                                   // not depend on which of the two it went through)
        const f32x2 sqc = raw2[j + 2] * raw2[j + 2];
        const float c = psb + sqc[0];
        f32x2 w = {c + psa, (c + sqa[1]) + sqc[1]};
        const f32x2 sc = __builtin_elementwise_fma(w, f32x2{1e-4f / 5.f, 1e-4f / 5.f}, f32x2{1.f, 1.f});
        const float r0 = __builtin_amdgcn_rsqf(sc[0]), r1 = __builtin_amdgcn_rsqf(sc[1]);   // v_rsq_f32 / v_sqrt_f32: 1 ulp, sc >= 1
        const f32x2 y = raw2[j + 1] * (f32x2{r0, r1} * f32x2{__builtin_amdgcn_sqrtf(r0), __builtin_amdgcn_sqrtf(r1)});
        Cs[lc0 + 2 * j + 2][lp] = y[0];
        Cs[lc0 + 2 * j + 3][lp] = y[1];
        sqa = sqb; psa = psb; sqb = sqc; psb = sqc[0] + sqc[1];
    };
    // 3x3 / stride 2 max pool: one thread per (channel, pooled row) = 8 outputs from 3 x 17 values; the column maxima are
    // shared by neighbouring windows.  Caffe clips windows at the blob's edge: positions beyond it hold 0 here (see the
    // v_med3 below) and every real value is >= 0 after the ReLU, so the plain maximum equals the clipped window's.
    float cm[C1_PC], pv[2][3];
    auto pool_fetch = [&](int q) {
        pv[q & 1][0] = pool_src[q]; pv[q & 1][1] = pool_src[C1_PC + q]; pv[q & 1][2] = pool_src[2 * C1_PC + q];
    };
    auto pool_col = [&](int q) { cm[q] = __builtin_fmaxf(__builtin_fmaxf(pv[q & 1][0], pv[q & 1][1]), pv[q & 1][2]); };
    auto pool_out = [&](int t) {
        const int pc = t % C1_TC, pr = (t / C1_TC) % C1_TR, b = t / (C1_TC * C1_TR);
        const int ph = C1_QR * pr + ppy;
        if (tid < 96 * C1_QR && ph < C1_POOL) {
            float* o = out + ((size_t)b * 96 + pk) * OHp * OWp + (size_t)(ph + opad) * OWp + C1_QC * pc + opad;
#pragma unroll
            for (int px = 0; px < C1_QC; ++px)
                if (C1_QC * pc + px < C1_POOL) o[px] = __builtin_fmaxf(__builtin_fmaxf(cm[2 * px], cm[2 * px + 1]), cm[2 * px + 2]);
        }
    };
    const int ccol = wave * 16 + c16;                                // this lane's column of the patch = position (crow, cc17)
    const int crow = ccol / C1_PC, cc17 = ccol - crow * C1_PC;
#ifdef C1D_TIME
    long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = (long long)__builtin_amdgcn_s_memtime();
#endif
    for (int it = 0; tile < total_tiles; ++it) {
        int nx = 0;
        if (tid == 0) nx = atomicAdd(tile_counter, 1);            // consumed at the end of the tile: its round trip is never waited for
        if (next < total_tiles) patch_load(next, pre, pre8);        // in flight under the MFMAs below
        f32x4 acc[6];
        // The operands of K step s + 1 are requested before the MFMAs of step s are issued (the scheduling barriers keep
        // the compiler from sinking the LDS reads back down to their first use, which leaves one LDS round trip exposed
        // in front of every pair of MFMAs).
        f32x2 av[2][3];
        float bv[2];
        auto operands = [&](int s2) {
            bv[s2 & 1] = *kb[s2];
            av[s2 & 1][0] = a0[2 * s2 * C1D_ALD]; av[s2 & 1][1] = a1[2 * s2 * C1D_ALD]; av[s2 & 1][2] = a2[2 * s2 * C1D_ALD];
        };
        operands(0);
        lrn_squares();
        // ---- first half of the K loop, with the previous tile's LRN (on the first tile: of zeros, unused) ----
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
            operands(s2 + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 6; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s2 & 1][i >> 1][i & 1], bv[s2 & 1], s2 ? acc[i] : bl[i], 0, 0, 0);
            if (s2 < 12) lrn_two(s2);
            __builtin_amdgcn_sched_barrier(0);
        }
        C1D_T(0)
        lds_barrier();                                              // the normalised patch is complete
        C1D_T(1)
        // ---- second half, with the previous tile's pooling (its LDS reads one step ahead of their use) ----
        pool_fetch(0);
#pragma unroll
        for (int s2 = 16; s2 < C1D_KS; ++s2) {
            if (s2 + 1 < C1D_KS) operands(s2 + 1);
            if (s2 - 15 < C1_PC) pool_fetch(s2 - 15);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 6; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s2 & 1][i >> 1][i & 1], bv[s2 & 1], acc[i], 0, 0, 0);
            pool_col(s2 - 16);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int q = C1D_KS - 15; q < C1_PC; ++q) pool_fetch(q);
#pragma unroll
        for (int q = C1D_KS - 16; q < C1_PC; ++q) pool_col(q);
        if (ptile >= 0) pool_out(ptile);
        C1D_T(2)
        lds_barrier();                                              // Cs and the raw patch are free
        C1D_T(3)
        if (next < total_tiles) patch_store(pre, pre8);
        // ---- ReLU -> LDS patch [channel][column] (bias is already in); positions outside the conv blob become 0 ----
        {
            const int pc = tile % C1_TC, pr = (tile / C1_TC) % C1_TR;
            const bool inside = ccol < C1_PR * C1_PC && (C1_PR - 1) * pr + crow < C1_OUT && (C1_PC - 1) * pc + cc17 < C1_OUT;
            const float cap = inside ? 3.402823466e38f : 0.f;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)                         // accumulator register r holds row 4 (lane / 16) + r
                    Cs[16 * i + 4 * g + r + 2][ccol] = __builtin_amdgcn_fmed3f(acc[i][r], 0.f, cap);
        }
        C1D_T(4)
        lds_barrier();
        C1D_T(5)
#pragma unroll
        for (int k = 0; k < 14; ++k)                                // all read before anything is written in place; rows 0, 1, 98, 99
            raw2[k] = f32x2{Cs[lc0 + 2 * k][lp], Cs[lc0 + 2 * k + 1][lp]};   //  are the zero halo
        if (tid == 0) s_next[(it + 1) & 1] = nx + (int)gridDim.x;
        C1D_T(6)
        lds_barrier();                                              // every raw value has been read; next tile index visible
        C1D_T(7)
        ptile = tile;
        tile = next;
        next = __builtin_amdgcn_readfirstlane(s_next[(it + 1) & 1]);
    }
    if (ptile >= 0) {                                               // drain: the last tile's epilogue
        lrn_squares();
#pragma unroll
        for (int j = 0; j < 12; ++j) lrn_two(j);
        lds_barrier();
#pragma unroll
        for (int q = 0; q < C1_PC; ++q) { pool_fetch(q); pool_col(q); }
        pool_out(ptile);
    }
#ifdef C1D_TIME
    if (lane == 0 && blockIdx.x < 256)
        for (int i = 0; i < 8; ++i) c1d_dbg[(blockIdx.x * 8 + wave) * 8 + i] = tacc[i];
#endif
}
#ifdef C1D_TIME
extern "C" int vpk_dbg_c1d(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(c1d_dbg), sizeof(long long) * 256 * 8 * 8); }
#endif

// conv1 input for the unfused / tapped paths (the default conv1_direct_kernel converts in its patch loader):
// float(uint8 raster) - mean (evaluation.py:35), written as the 16 stride-4 phase planes (Px = float: float image - mean)
//   P[py][px][Y][X] = x[4Y + py][4X + px]   (125 x 125 each)
// so that conv1 (11 x 11, stride 4) is a stride-1 gather for the DMA kernel: tap (kh, kw) of output (oh, ow)
// is P[kh % 4][kw % 4][oh + kh / 4][ow + kw / 4], and the 64 lanes of a gather (consecutive ow) read 256
// contiguous bytes instead of 64 words 16 bytes apart (8-16 cache lines per gather).  Measured (r1): conv1
// 2.76 -> 2.57 ms at B = 512, unchanged at B = 102.  With its MFMAs and stores removed conv1 still takes
// 0.36 of its 0.58 ms: with only 8 K-stages per tile it is bound by the issue rate of the 4-byte gather DMAs
// (about one per 40-60 cycles per CU), which a wider (16-byte, row-tiled) loader would relieve.
template <typename Px>
__global__ void prep_input_kernel(const Px* __restrict__ sphere, const float* __restrict__ mean,
                                  float* __restrict__ out, int plane) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;       // pixel within the image
    if (p >= plane) return;
    const size_t img = (size_t)blockIdx.y * plane;             // blockIdx.y = image
    const int y = p / 500, x = p - y * 500;
    const int q = ((y % C1_PH) * C1_PH + (x % C1_PH)) * (C1_PW * C1_PW) + (y / C1_PH) * C1_PW + x / C1_PH;
    out[img + q] = (float)sphere[img + p] - mean[p];
}

// sum the split-K partials, add bias, activation: act 0 = none, 1 = ReLU, 2 = sigmoid
__global__ void splitk_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias, int ksplit,
                                     long long N, int OC, int act, float* __restrict__ out, float* __restrict__ pre,
                                     const int* __restrict__ live) {
    if (live) N = *live;                                       // recompute pass: the partials of the device count's images
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * OC) return;
    int m = (int)(idx % OC);
    float v = 0.f;
    for (int s = 0; s < ksplit; ++s) v += part[(size_t)s * N * OC + idx];
    v += bias[m];
    if (pre) pre[idx] = v;
    if (act == 1) v = v > 0.f ? v : 0.f;
    else if (act == 2) v = 1.f / (1.f + expf(-v));          // Sigmoid layer (deploy.prototxt:298-304)
    out[idx] = v;
}


// Fused LRN (across channels, local_size 5, x * (1 + alpha/n * sum x^2)^-beta) + MAX pool 3x3 stride 2, ceil
// mode with clipped windows (deploy.prototxt:34-55, 82-103): the normalised map (0.6 GB at B = 102 for
// norm1) is never written to or re-read from HBM.
constexpr int LRN_CCH = 16;   // channels per workgroup (plus a 2-channel halo on each side)
// A workgroup owns TPH x TPW pooled outputs of 16 channels.
//   1. the raw input patch ((2 TPH + 1) x (2 TPW + 1) pixels, 16 + 4 halo channels) goes to LDS;
//   2. one thread per pixel walks the channels with a 5-deep register window and overwrites the patch in
//      place with the normalised values -- every pixel is normalised ONCE (a thread per pooled output
//      normalises each of its 9 taps itself: 2.25x the work and 9 dependent global loads per channel);
//   3. 3x3 / stride 2 max over the patch in LDS (window clipped at the border like Caffe), written into the
//      next convolution's bordered planes.
// norm2 + pool2 as a STREAM over the channels (r3).  The tiled kernel below gives a workgroup 16 channels of a small
// spatial patch: 20 / 16 of the channels and 13 x 31 / (12 x 30) of the pixels are read, in 124-byte row pieces, and it
// ran at 0.28 of the HBM rate.  Here a workgroup owns TPH pooled rows x the WHOLE width of one image -- in an unpadded
// NCHW plane that is one contiguous run of (2 TPH + 1) W floats per channel -- and walks a range of C / cgroups channels
// (plus two raw channels either side to start and end the window): a thread keeps
// the 5-deep raw window of its (up to four) pixels in registers, so every raw value is read exactly once, fully
// coalesced, CB channels (32 loads per thread) in flight; the normalised planes of a batch go to LDS (double buffered:
// one barrier per batch), the 3 x 3 / 2 maxima come out of LDS with Caffe's clipped windows and are written with the next
// convolution's border.  Same expressions in the same order as the tiled kernel: the same bits.
template <int TPH, int CB>
__global__ __launch_bounds__(256) void lrn5_pool3s2_stream_kernel(const float* __restrict__ in, float* __restrict__ out, int C,
                                                                  int H, int W, int PH, int PW, float alpha, float beta,
                                                                  int PHp, int PWp, int opad, int cgroups, const int* __restrict__ live) {
    constexpr int TR = 2 * TPH + 1, SLOTS = 4, PMAX = 256 * SLOTS;
    __shared__ float plane[2][CB][PMAX];
    const int tiles_h = (PH + TPH - 1) / TPH;
    const int th = blockIdx.x % tiles_h, cgi = (blockIdx.x / tiles_h) % cgroups, b = blockIdx.x / (tiles_h * cgroups);
    if (live && b >= *live) return;                      // (recompute pass: slots beyond the device count)
    const int cper = C / cgroups, c_lo = cgi * cper, c_hi = c_lo + cper;      // this workgroup's channels [c_lo, c_hi)
    const int ph0 = th * TPH, h0 = 2 * ph0;
    const int HW = H * W, npix = TR * W;                 // npix <= PMAX (checked by the host)
    const float* x = in + (size_t)b * C * HW + (size_t)h0 * W;
    bool ok[SLOTS];
    int off[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        off[i] = threadIdx.x + 256 * i;
        ok[i] = off[i] < npix && h0 + off[i] / W < H;    // (rows past the blob are zeros: they only meet clipped windows)
    }
    int ld_off[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) ld_off[i] = ok[i] ? off[i] : 0;
    float v0[SLOTS], v1[SLOTS], v2[SLOTS], v3[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {                    // raw values of the channels c_lo - 2 .. c_lo + 1 (zeros outside the blob)
        v0[i] = (ok[i] && c_lo >= 2) ? x[(size_t)(c_lo - 2) * HW + off[i]] : 0.f;
        v1[i] = (ok[i] && c_lo >= 1) ? x[(size_t)(c_lo - 1) * HW + off[i]] : 0.f;
        v2[i] = ok[i] ? x[(size_t)c_lo * HW + off[i]] : 0.f;
        v3[i] = (ok[i] && c_lo + 1 < C) ? x[(size_t)(c_lo + 1) * HW + off[i]] : 0.f;
    }
    const float an = alpha / 5.f;
    int buf = 0;
    float nx[CB][SLOTS], nn[CB][SLOTS];                  // raw values of this batch's / the next batch's channels (+2)
    auto fetch = [&](int cb, float (&dst)[CB][SLOTS]) {
#pragma unroll
        for (int k = 0; k < CB; ++k)
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) {            // unconditional loads (clamped addresses) first, all of them in flight ...
                const int c4 = cb + k + 2;
                dst[k][i] = x[(size_t)(c4 < C ? c4 : C - 1) * HW + ld_off[i]];
            }
    };
    auto mask = [&](int cb, float (&dst)[CB][SLOTS]) {    // ... zeroed where there is no such pixel / channel when they are used
#pragma unroll
        for (int k = 0; k < CB; ++k)
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) dst[k][i] = (ok[i] && cb + k + 2 < C) ? dst[k][i] : 0.f;
    };
    fetch(c_lo, nx);
    for (int cb = c_lo; cb < c_hi; cb += CB) {
        fetch(cb + CB, nn);                              // the next batch's loads are in flight under this batch's work
        mask(cb, nx);
#pragma unroll
        for (int k = 0; k < CB; ++k)
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) {
                const float v4 = nx[k][i];
                const float sc = 1.f + an * (v0[i] * v0[i] + v1[i] * v1[i] + v2[i] * v2[i] + v3[i] * v3[i] + v4 * v4);
                float pw_;
                if (beta == 0.75f) {
                    const float r = __builtin_amdgcn_rsqf(sc);
                    pw_ = r * __builtin_amdgcn_sqrtf(r);
                }
                else pw_ = powf(sc, -beta);
                if (off[i] < PMAX) plane[buf][k][off[i]] = v2[i] * pw_;
                v0[i] = v1[i]; v1[i] = v2[i]; v2[i] = v3[i]; v3[i] = v4;
            }
#pragma unroll
        for (int k = 0; k < CB; ++k)
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) nx[k][i] = nn[k][i];
        __syncthreads();
        for (int e = threadIdx.x; e < CB * TPH * PW; e += 256) {
            const int k = e / (TPH * PW), o = e - k * (TPH * PW);
            const int oy = o / PW, ox = o - oy * PW;
            const int ph = ph0 + oy, c = cb + k;
            if (ph >= PH || c >= c_hi) continue;
            float m = -3.402823466e38f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int r = 2 * oy + dy, q = 2 * ox + dx;
                    if (h0 + r < H && q < W) {            // Caffe clips the window at the border
                        const float v = plane[buf][k][r * W + q];
                        m = v > m ? v : m;
                    }
                }
            out[((size_t)b * C + c) * PHp * PWp + (size_t)(ph + opad) * PWp + ox + opad] = m;
        }
        buf ^= 1;
    }
}

template <int TPH, int TPW>
__global__ __launch_bounds__(256) void lrn5_pool3s2_tiled_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                 int C, int H, int W, int PH, int PW, float alpha,
                                                                 float beta, int PHp, int PWp, int opad) {
    constexpr int CC = LRN_CCH, NPL = CC + 4;
    constexpr int TR = 2 * TPH + 1, TC = 2 * TPW + 1, NPIX = TR * TC;
    __shared__ float patch[NPL][NPIX];
    const int tiles_w = (PW + TPW - 1) / TPW, tiles_h = (PH + TPH - 1) / TPH;
    const int nch = (C + CC - 1) / CC;
    int bid = blockIdx.x;
    const int tw = bid % tiles_w; bid /= tiles_w;
    const int th = bid % tiles_h; bid /= tiles_h;
    const int ch = bid % nch;
    const int b = bid / nch;
    const int c0 = ch * CC;
    const int ph0 = th * TPH, pw0 = tw * TPW;
    const int h0 = 2 * ph0, w0 = 2 * pw0;
    const int HW = H * W;
    const float* x = in + (size_t)b * C * HW;
    // 1. raw patch (zeros outside the blob: they only ever meet clipped windows or the LRN's zero padding)
    constexpr int LU = 8;                               // loads in flight per thread (the loop is latency-bound without them)
    for (int e0 = threadIdx.x; e0 < NPL * NPIX; e0 += 256 * LU) {
        float v[LU];
#pragma unroll
        for (int u = 0; u < LU; ++u) {
            const int e = e0 + u * 256;
            const int pl = e / NPIX, p = e - pl * NPIX;
            const int r = p / TC, q = p - r * TC;
            const int c = c0 - 2 + pl, h = h0 + r, w = w0 + q;
            v[u] = 0.f;
            if (e < NPL * NPIX && c >= 0 && c < C && h < H && w < W) v[u] = x[(size_t)c * HW + (size_t)h * W + w];
        }
#pragma unroll
        for (int u = 0; u < LU; ++u) {
            const int e = e0 + u * 256;
            if (e < NPL * NPIX) patch[0][e] = v[u];     // patch is contiguous: [pl][p] == flat e
        }
    }
    __syncthreads();
    // 2. normalise in place, one thread per pixel
    const float an = alpha / 5.f;
    for (int p = threadIdx.x; p < NPIX; p += 256) {
        float v0 = patch[0][p], v1 = patch[1][p], v2 = patch[2][p], v3 = patch[3][p];
#pragma unroll
        for (int k = 0; k < CC; ++k) {
            const float v4 = patch[k + 4][p];
            const float sc = 1.f + an * (v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3 + v4 * v4);
            float pw_;
            if (beta == 0.75f) {                         // v_rsq_f32 / v_sqrt_f32 (1 ulp, sc >= 1); the IEEE-exact library
                const float r = __builtin_amdgcn_rsqf(sc);   // forms expand to ~25 VALU instructions each
                pw_ = r * __builtin_amdgcn_sqrtf(r);
            }
            else pw_ = powf(sc, -beta);
            patch[k + 2][p] = v2 * pw_;                  // plane k+2 holds channel c0+k; its raw value lives in v2
            v0 = v1; v1 = v2; v2 = v3; v3 = v4;
        }
    }
    __syncthreads();
    // 3. pool
    for (int e = threadIdx.x; e < CC * TPH * TPW; e += 256) {
        const int k = e / (TPH * TPW), o = e - k * (TPH * TPW);
        const int oy = o / TPW, ox = o - oy * TPW;
        const int ph = ph0 + oy, pw = pw0 + ox, c = c0 + k;
        if (ph >= PH || pw >= PW || c >= C) continue;
        float m = -3.402823466e38f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int r = 2 * oy + dy, q = 2 * ox + dx;
                if (h0 + r < H && w0 + q < W) {          // Caffe clips the window at the border
                    const float v = patch[k + 2][r * TC + q];
                    m = v > m ? v : m;
                }
            }
        out[((size_t)b * C + c) * PHp * PWp + (size_t)(ph + opad) * PWp + pw + opad] = m;
    }
}

// pool5 (deploy.prototxt:181-191): 3 x 3 / 2 max pool of unpadded 30 x 30 planes -> 15 x 15 (ceil mode: the last window is
// clipped).  A workgroup stages PL whole planes in LDS with 16-byte loads (a plane is 3600 contiguous bytes; the windows
// of neighbouring outputs overlap, and one thread per output reading its nine values from HBM ran at 2.3 TB/s), then
// every thread takes pooled outputs out of LDS; stores are contiguous.  Maxima: order-free, same values.
template <int PL>
__global__ __launch_bounds__(256) void pool5_kernel(const float* __restrict__ in, float* __restrict__ out, long long planes,
                                                    const int* __restrict__ live) {
    constexpr int H = 30, W = 30, P = 15, HW = H * W, PP = P * P;
    __shared__ __attribute__((aligned(16))) float s[PL * HW];
    const long long p0 = (long long)blockIdx.x * PL;
    if (live && p0 >= (long long)*live * 256) return;    // (recompute pass: the 256 planes of each image beyond the device count)
    const int np = planes - p0 < PL ? (int)(planes - p0) : PL;
    const f32x4* src = reinterpret_cast<const f32x4*>(in + p0 * HW);
    for (int q = threadIdx.x; q < np * HW / 4; q += 256) reinterpret_cast<f32x4*>(s)[q] = src[q];
    __syncthreads();
    float* dst = out + p0 * PP;
    for (int e = threadIdx.x; e < np * PP; e += 256) {
        const int pl = e / PP, o = e - pl * PP;
        const int py = o / P, px = o - py * P;
        const float* x = s + pl * HW + (2 * py) * W + 2 * px;
        const bool by = 2 * py + 2 < H, bx = 2 * px + 2 < W;     // (only the last row / column of windows is clipped)
        float m = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[W], x[W + 1]));
        if (bx) m = fmaxf(m, fmaxf(x[2], x[W + 2]));
        if (by) m = fmaxf(m, fmaxf(x[2 * W], x[2 * W + 1]));
        if (bx && by) m = fmaxf(m, x[2 * W + 2]);
        dst[e] = m;
    }
}

// weight re-pack: Caffe [G*OC][K] (K contiguous) -> k-major panels [G][Kp][Mp], zero padded
__global__ void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ wp, int G, int OC, int K,
                                    int Kp, int Mp) {
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)G * Kp * Mp) return;
    int m = (int)(idx % Mp);
    int k = (int)((idx / Mp) % Kp);
    int g = (int)(idx / ((long long)Mp * Kp));
    wp[idx] = (m < OC && k < K) ? w[((size_t)g * OC + m) * K + k] : 0.f;
}

#include "cnn_split_gemm.hpp"
#include "cnn_pairs.hpp"
#include "cnn_conv1_pieces.hpp"
#include "cnn_conv_pieces.hpp"
#include "cnn_norm_pool_planes.hpp"
#include "cnn_dense_pieces.hpp"
#include "cnn_winograd.hpp"

struct Layer {
    ConvDims d;
    float* wp = nullptr;     // packed weights
    float* bias = nullptr;
    unsigned* ktab = nullptr;   // im2col table (conv layers): byte offset of tap k inside the padded input planes
    unsigned short* wsplit = nullptr;   // conv2..5: weights as three bf16 pieces in MFMA fragment order (cnn_split_gemm.hpp)
    float ascale = CP_DEFAULT_ASCALE;   // conv2..5, fc6, fc7 on fp16 pairs: the power of two the layer's INPUT is multiplied by (calibrate())
    float hscale = 1.f;                 // conv2..5, fc6, fc7: the power of two the weights are multiplied by before the fp16 split (largest in [2^13, 2^14))
    unsigned short* whalf = nullptr;    // conv2..5: weights as scaled fp16 pairs in the same order (cnn_conv_pieces.hpp, NP = 2)
    PieceDims pdh;                      //            and the layer's dimensions for that path (own block padding, output scale)
    SplitDims sd;
    float* wino = nullptr;      // conv2..5: G g G^T in the chunk order of the Winograd kernels (cnn_winograd.hpp)
    unsigned short* c1frag = nullptr;   // conv1: three bf16 pieces of every weight in MFMA fragment order (cnn_conv1_pieces.hpp)
    unsigned short* c1half = nullptr;   // conv1: scaled fp16 pairs in the same order (c1scale: the power of two)
    float c1scale = 1.f;
    float* c1map = nullptr;     // conv1: bias - conv1(mean), 123 x 123 x 96
    WinoDims wd;
    Wino5Dims wd5;
    PieceDims pd;               // conv2..5 on exact bf16 pieces from an LDS-resident patch (cnn_conv_pieces.hpp)
    float* wraw = nullptr;      // fc6, fc7: the f32 weights in tile order (dense_tile_weights_kernel), streamed by dense_pieces_kernel (cnn_dense_pieces.hpp)
    unsigned short* wpair = nullptr;   // fc6, fc7: the same weights as scaled fp16 pairs in A-fragment order (dense_pair_weights_kernel): the default's stream
};

int ceil_pool(int in, int k, int s) { return (in - k + s - 1) / s + 1; }

}  // namespace

struct vpk_cnn_state {
    Layer L[8];              // conv1..5, fc6..8
    float* mean = nullptr;
    bool loaded = false;
    // activations (grown on demand)
    float* act = nullptr;
    size_t act_bytes = 0;
    int act_batch = 0;
    unsigned short* xfrag = nullptr;   // fc6's input as bf16 B fragments (dense_split_kernel), grown on demand
    size_t xfrag_bytes = 0;
    unsigned* range_word = nullptr;    // fp16 pairs: bit li set when a scaled INPUT value of layer li reached fp16's range (split2h_guard);
                                       // sticky until vpk_cnn_range_flags reads and clears it.  range_word[1]: where the pair pass
                                       // reports under RECOMPUTE_EXACT (its flagged images are recomputed, so nothing reaches word 0)
    // range policy (vpk_cnn_set_range_policy): 0 = RAISE, 1 = RECOMPUTE_EXACT
    int range_policy = 0;
    unsigned* img_range = nullptr;     // the last vpk_cnn_forward's per-image bits (image b at [b]), grown on demand
    size_t img_range_bytes = 0;
    int img_range_batch = 0;           // its batch (0: no forward yet)
    int* rc_list = nullptr;            // recompute pass: [0] = device count of flagged images of the chunk, [1 ..] their indices in order
    unsigned long long* rc_total = nullptr;   // images recomputed since vpk_cnn_recomputed last read it
    // optional per-layer timing (HIP events on the handle's stream)
    int split_variant = 0;   // (development) tiling of the split GEMM
    int precision = 0;       // vpk_cnn_set_precision: 0 = native f32 MFMA, 1 = conv2..5 on the bf16 matrix cores (3-piece split)
    int algorithm = 4;       // vpk_cnn_set_algorithm: 4 = conv2..5 / fc6 on scaled fp16 pairs (default), 2 = conv2 / fc6 on bf16 triples + Winograd, ...
                             // direct convolutions on exact bf16 pieces (cnn_conv_pieces.hpp)
    int fuse_conv1 = 3;      // conv1 + norm1 + pool1 as one kernel (vpk_cnn_set_fusion): 0 = separate kernels, 1 = direct f32,
                             // 2 = GEMM-fused, 3 (default) = direct on the bf16 matrix cores with exact operands
    int conv1_group = 4;     // images per work item of conv1_pieces_kernel (VPK_CONV1_GROUP: development knob)
    int dense_presplit = 1;  // fc6 / fc7 on fp16 pairs: stream the pre-split fragments (VPK_DENSE_PRESPLIT=0: split the f32 stream in registers, round 5)
    bool profiling = false;
    static constexpr int EV_RING = 64;   // event sets of the last 64 profiled passes (vpk_cnn_mean_layer_ms)
    hipEvent_t ev[EV_RING][14] = {};
    long long ev_pass = 0;   // profiled passes recorded since profiling was switched on
    bool ev_ready = false;
    bool ev_valid = false;
};

void vpk_cnn_free(vpk_handle* h) {
    if (!h->cnn) return;
    for (auto& l : h->cnn->L) {
        if (l.wp) (void)hipFree(l.wp);
        if (l.bias) (void)hipFree(l.bias);
        if (l.ktab) (void)hipFree(l.ktab);
        if (l.wsplit) (void)hipFree(l.wsplit);
        if (l.whalf) (void)hipFree(l.whalf);
        if (l.wino) (void)hipFree(l.wino);
        if (l.c1frag) (void)hipFree(l.c1frag);
        if (l.c1half) (void)hipFree(l.c1half);
        if (l.c1map) (void)hipFree(l.c1map);
        if (l.wraw) (void)hipFree(l.wraw);
        if (l.wpair) (void)hipFree(l.wpair);
    }
    if (h->cnn->mean) (void)hipFree(h->cnn->mean);
    if (h->cnn->act) (void)hipFree(h->cnn->act);
    if (h->cnn->xfrag) (void)hipFree(h->cnn->xfrag);
    if (h->cnn->range_word) (void)hipFree(h->cnn->range_word);
    if (h->cnn->img_range) (void)hipFree(h->cnn->img_range);
    if (h->cnn->rc_list) (void)hipFree(h->cnn->rc_list);
    if (h->cnn->rc_total) (void)hipFree(h->cnn->rc_total);
    if (h->cnn->ev_ready)
        for (auto& set : h->cnn->ev)
            for (auto& e : set) (void)hipEventDestroy(e);
    delete h->cnn;
    h->cnn = nullptr;
}

namespace {

// static topology of cnn/deploy.prototxt (per-group channel counts).  H, W = unpadded input plane,
// P = convolution padding (the input planes are stored with that zero border), OP = border of the
// OUTPUT planes (= padding of the layer that consumes them; 0 = dense).
struct Topo { int IC, H, W, OC, OH, OW, G, KH, S, P, BM, OP; };
constexpr Topo TOPO[8] = {
    {1, 500, 500, 96, 123, 123, 1, 11, 4, 0, 96, 0},     // conv1 (:9-27)      -> LRN/pool (dense)
    {48, 61, 61, 128, 61, 61, 2, 5, 1, 2, 128, 0},       // conv2 (:56-75) g2  -> LRN/pool (dense)
    {256, 30, 30, 384, 30, 30, 1, 3, 1, 1, 128, 1},      // conv3 (:104-122)   -> conv4 (pad 1)
    {192, 30, 30, 192, 30, 30, 2, 3, 1, 1, 96, 1},       // conv4 (:129-148) g2 -> conv5 (pad 1)
    {192, 30, 30, 128, 30, 30, 2, 3, 1, 1, 128, 0},      // conv5 (:155-174) g2 -> pool5 (dense)
    {57600, 1, 1, 4096, 1, 1, 1, 1, 1, 0, 128, 0},       // fc6 (:192-210)
    {4096, 1, 1, 4096, 1, 1, 1, 1, 1, 0, 128, 0},        // fc7 (:224-242)
    {4096, 1, 1, 400, 1, 1, 1, 1, 1, 0, 128, 0},         // fc8_20x20 (:257-275)
};
// split-K of the dense layers.  fc6: 32 m-tiles x 72 = 2304 tiles of 50 K-steps for the 768 resident workgroups' queue: with
// 24 (one tile per workgroup) the layer took 0.40 ms alone but 0.79 ms beside the EM -- the workgroups of the ~166 free CUs
// each needed a second whole tile --, with 72 it takes 0.40 / 0.66 ms (round 4; the partials grow from 40 to 120 MB)
constexpr int KSPLIT[8] = {1, 1, 1, 1, 1, 72, 16, 32};
constexpr size_t splitk_partials_per_image() {          // the partials region: max over the dense layers of ksplit x outputs
    size_t m = 0;
    for (int li = 5; li < 8; ++li) m = (size_t)KSPLIT[li] * TOPO[li].OC > m ? (size_t)KSPLIT[li] * TOPO[li].OC : m;
    return m;
}

// Activation arena: one region per blob, floats per image.  Regions are carved by the CAPACITY batch,
// so an image's planes sit at the same address for every batch size <= capacity and the zero borders
// written at allocation time stay valid.  Nothing is reused between layers (17.6 MB per image; 288 GB
// of HBM3E makes ping-pong buffers unnecessary, and the borders must not be overwritten).
enum Region { R_IN, R_CONV1, R_POOL1, R_CONV2, R_POOL2, R_CONV3, R_CONV4, R_CONV5, R_POOL5, R_FCA, R_FCB, R_PART, R_SPLIT, R_SPLIT4, R_SPLIT5, R_P6_2, R_P6_3, R_P6_5, R_COUNT };
constexpr int MAX_CHUNK = 4096;     // images per run_forward at most (32-bit positions inside one launch)
constexpr size_t CTR_FLOATS = 64;   // tile-queue counters of the 8 GEMM launches, behind the regions
constexpr size_t GUARD_FLOATS = 64;  // between the last region and the counters: conv_pieces_kernel's patch DMA reads up to 8 words (128
                                     // bytes) past a plane's last row (columns that are never stored); for the last plane of the last
                                     // image of the last region that must be zeros of the arena, not live counters
static_assert(GUARD_FLOATS * sizeof(float) >= 8 * 16, "the patch DMA's overrun: 8 words of 16 bytes");
constexpr size_t REGION_FLOATS[R_COUNT] = {
    500ull * 500,            // fp32 input (raster - mean)
    96ull * 123 * 123,       // conv1, dense
    96ull * 65 * 65,         // pool1 with conv2's border of 2
    256ull * 61 * 61,        // conv2, dense
    256ull * 32 * 32,        // pool2 with conv3's border of 1
    384ull * 32 * 32,        // conv3 with conv4's border
    384ull * 32 * 32,        // conv4 with conv5's border
    256ull * 900,            // conv5, dense
    256ull * 225,            // pool5 = fc6 input
    4096, 4096,              // fc6 / fc7 outputs
    splitk_partials_per_image(),   // split-K partials (fc6: 72 x 4096 floats = 1.2 MB per capacity image)
    96ull * 65 * 65 * 3 / 2, // the current conv layer's input as three bf16 NHWC pieces (largest: pool1)
    384ull * 32 * 32 * 3 / 2, // conv4's / conv5's input in that format, written by the previous layer's epilogue (interior
    384ull * 32 * 32 * 3 / 2, //  only: the zero border comes from the arena's allocation)
    96ull * 65 * 65 * 3 / 2,  // conv2's input as P6 planes (cnn_conv_pieces.hpp: [channel group][piece x k half][y][x] 16-byte words)
    256ull * 32 * 32 * 3 / 2, // conv3's (vpk_cnn_set_algorithm(3) only: measurements)
    384ull * 32 * 32 * 3 / 2, // conv5's (vpk_cnn_set_algorithm(3) only: measurements)
};
constexpr size_t arena_floats_per_image() {
    size_t t = 0;
    for (int i = 0; i < R_COUNT; ++i) t += REGION_FLOATS[i];
    return t;
}
// dense sizes of the blobs a tap can return
constexpr size_t A_CONV1 = 96ull * 123 * 123, A_POOL1 = 96ull * 61 * 61;
constexpr size_t A_CONV2 = 256ull * 61 * 61, A_POOL2 = 256ull * 30 * 30;
constexpr size_t A_CONV3 = 384ull * 900, A_CONV4 = 384ull * 900, A_CONV5 = 256ull * 900, A_POOL5 = 256ull * 225;
constexpr size_t A_FC6 = 4096, A_FC7 = 4096, A_FC8 = 400;

// interior of bordered planes -> dense (taps only)
__global__ void unpad_kernel(const float* __restrict__ in, float* __restrict__ out, long long planes, int H, int W,
                             int Hp, int Wp, int pad) {
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= planes * H * W) return;
    const int w = (int)(idx % W), hh = (int)((idx / W) % H);
    const long long pl = idx / ((long long)W * H);
    out[idx] = in[((size_t)pl * Hp + hh + pad) * Wp + w + pad];
}

template <typename KernelT>
void launch_dma(vpk_handle* h, KernelT kernel, const ConvDims& d, int BM, const float* in, const Layer& l, float* out,
                int stride, int* counter, int wpc = 3, const int* live = nullptr) {
    long long ntiles = (d.N + 127) / 128;
    long long total = (long long)d.groups * d.ksplit * ntiles * (d.Mp / BM);
    long long blocks = std::min<long long>(total, (long long)wpc * h->num_cu);   // wpc workgroups fit a CU (LDS, registers)
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(CONV_THREADS), 0, h->stream, d, in, l.wp, l.bias, l.ktab,
                       out, stride, counter, (int)total, live);
}

// Where a forward reports what its fp16-pair writers clamp, and which images it runs (vpk_cnn_set_range_policy).
struct FwdCtl {
    unsigned* range_word;       // the sticky word the pair writers OR the consuming layer's bit into
    unsigned* img_range;        // the same bits per image of this launch (image b at img_range[b]); null: not kept
    const int* live;            // recompute pass: the device count of images -- `batch` is then only its upper bound; null: batch
};

// The images of a forward: uint8 rasters (vpk_cnn_forward) or float images before the mean (vpk_cnn_forward_f32), B x 500 x 500
struct Images {
    const void* p;
    bool f32;
    const uint8_t* u8() const { return static_cast<const uint8_t*>(p); }
    const float* f() const { return static_cast<const float*>(p); }
    Images at(size_t b) const { return Images{f32 ? (const void*)(f() + b * 250000) : (const void*)(u8() + b * 250000), f32}; }
};

int run_forward(vpk_handle* h, Images img, int batch, float* out, int tap, float* tap_out, const FwdCtl& fc) {
    vpk_cnn_state* S = h->cnn;
    hipStream_t st = h->stream;
    // the kernels that honour a device count are those of the exact configuration with the default conv1
    if (fc.live && !(S->precision == 0 && S->algorithm == 2 && S->fuse_conv1 == 3 && tap < 0 && !S->profiling))
        return vpk_fail(h, VPK_ERR_STATE, "run_forward: a device-counted pass runs algorithm 2 with the default conv1, untapped");
    const int* live = fc.live;
    // (the scaled fp16-pair conv1 relies on a pixel being an exact fp16 number: uint8 rasters only)
    if (img.f32 && S->fuse_conv1 == 4 && !(tap == 0 || !S->fuse_conv1))
        return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_forward_f32: vpk_cnn_set_fusion(4) takes uint8 rasters only");
    if (batch > S->act_batch) {     // grow the arena; all borders (and everything else) start as zeros
        const size_t need = ((size_t)batch * arena_floats_per_image() + GUARD_FLOATS + CTR_FLOATS) * sizeof(float);
        int rc = vpk_reserve(h, (void**)&S->act, &S->act_bytes, need, "hipMalloc(CNN activations)");
        if (rc) return rc;
        VPK_HIP(h, hipMemsetAsync(S->act, 0, need, st));
        S->act_batch = batch;
    }
    float* R[R_COUNT];
    {
        size_t off = 0;
        for (int i = 0; i < R_COUNT; ++i) { R[i] = S->act + off; off += (size_t)S->act_batch * REGION_FLOATS[i]; }
    }
    int* ctr = reinterpret_cast<int*>(S->act + (size_t)S->act_batch * arena_floats_per_image() + GUARD_FLOATS);
    VPK_HIP(h, hipMemsetAsync(ctr, 0, CTR_FLOATS * sizeof(float), st));
    auto tapcopy = [&](int id, const float* src, size_t per) -> int {
        if (tap == id && tap_out)
            VPK_HIP(h, hipMemcpyAsync(tap_out, src, per * batch * sizeof(float), hipMemcpyDeviceToDevice, st));
        return VPK_OK;
    };
    auto ew_blocks = [](long long n) { return (unsigned)((n + 255) / 256); };
    auto tapunpad = [&](int id, const float* src, int C, int H, int W, int pad) {
        if (tap == id && tap_out) {
            const long long planes = (long long)batch * C;
            hipLaunchKernelGGL(unpad_kernel, dim3(ew_blocks(planes * H * W)), dim3(256), 0, st, src, tap_out, planes, H, W,
                               H + 2 * pad, W + 2 * pad, pad);
        }
    };
    auto dims = [&](int li) {
        ConvDims d = S->L[li].d;
        d.B = batch;
        d.N = batch * d.OH * d.OW;
        return d;
    };
    int evi = 0;
    hipEvent_t* evs = S->ev[S->ev_pass % vpk_cnn_state::EV_RING];
    auto mark = [&]() {
        if (S->profiling && evi < 14) (void)hipEventRecord(evs[evi++], st);
    };
    int rc;
    mark();

    // (conv1's fused kernel on pieces hands conv2 its input planes when conv2 runs on fp16 pairs and nobody asks for pool1)
    const bool conv1_hands_planes = S->precision == 0 && S->algorithm == 4 && S->fuse_conv1 >= 3 && tap != 0 && tap != 1;
    // conv1 + relu1: uint8 raster - mean -> fp32 (pre-pass), then the DMA kernel
    const bool direct = !(tap == 0 || !S->fuse_conv1) && S->fuse_conv1 != 2;   // conv1_direct_kernel reads the rasters itself
    if (!direct) {
        if (img.f32)
            hipLaunchKernelGGL(prep_input_kernel<float>, dim3((500 * 500 + 255) / 256, batch), dim3(256), 0, st, img.f(), S->mean, R[R_IN],
                               500 * 500);
        else
            hipLaunchKernelGGL(prep_input_kernel<unsigned char>, dim3((500 * 500 + 255) / 256, batch), dim3(256), 0, st, img.u8(), S->mean,
                               R[R_IN], 500 * 500);
    }
    if (tap == 0 || !S->fuse_conv1) {
        launch_dma(h, conv_gemm_dma_kernel<1, 4, 3, 1, false>, dims(0), 96, R[R_IN], S->L[0], R[R_CONV1], 1, ctr + 0);   // stride 1 over the phase planes
        mark();
        if ((rc = tapcopy(0, R[R_CONV1], A_CONV1))) return rc;
        // norm1 + pool1 (fused), written with conv2's border
        hipLaunchKernelGGL((lrn5_pool3s2_tiled_kernel<7, 16>), dim3((unsigned)(batch * ((96 + LRN_CCH - 1) / LRN_CCH) * 9 * 4)),
                           dim3(256), 0, st, R[R_CONV1], R[R_POOL1], 96, 123, 123, 61, 61, 1e-4f, 0.75f, 65, 65, 2);
        mark();
        mark();
    } else {
        // conv1 + relu1 + norm1 + pool1 in one kernel: 21 x 8 patches of 7 x 17 conv outputs per image, straight into
        // pool1's planes (with conv2's border of 2); the conv1 blob only exists when a caller taps it
        if (S->fuse_conv1 >= 3) {                         // exact bf16 pieces (3) / scaled fp16 pairs (4) on the matrix cores (cnn_conv1_pieces.hpp)
            const int group = S->conv1_group;
            const int total = C1B_PATCHES * ((batch + group - 1) / group);
            // fp16 pairs downstream and pool1 not tapped: the pooling stage writes conv2's piece planes itself (no f32 pool1 blob)
            unsigned short* c2planes = conv1_hands_planes ? reinterpret_cast<unsigned short*>(R[R_P6_2]) : nullptr;
            if (S->fuse_conv1 == 4)
                hipLaunchKernelGGL(conv1_pieces_kernel<2>, dim3((unsigned)std::min(total, h->num_cu)), dim3(C1B_THREADS), 0, st, img.u8(),
                                   S->L[0].c1half, S->L[0].c1map, R[R_POOL1], 65, 65, 2, batch, group, 1.f / S->L[0].c1scale, ctr + 0, total,
                                   c2planes, S->L[1].ascale, fc.range_word, fc.img_range, live);
            else if (img.f32)                             // float images: three pieces per pixel, six products per K step
                hipLaunchKernelGGL((conv1_pieces_kernel<3, float>), dim3((unsigned)std::min(total, h->num_cu)), dim3(C1B_THREADS), 0, st,
                                   img.f(), S->L[0].c1frag, S->L[0].c1map, R[R_POOL1], 65, 65, 2, batch, group, 1.f, ctr + 0, total,
                                   c2planes, S->L[1].ascale, fc.range_word, fc.img_range, live);
            else
                hipLaunchKernelGGL(conv1_pieces_kernel<3>, dim3((unsigned)std::min(total, h->num_cu)), dim3(C1B_THREADS), 0, st, img.u8(),
                                   S->L[0].c1frag, S->L[0].c1map, R[R_POOL1], 65, 65, 2, batch, group, 1.f, ctr + 0, total,
                                   c2planes, S->L[1].ascale, fc.range_word, fc.img_range, live);
        } else if (S->fuse_conv1 == 2) {                  // the implicit-GEMM kernel with the fused epilogue (kept for comparison)
            ConvDims df = dims(0);
            df.N = batch * C1_TR * C1_TC * 128;           // one 128-column tile per patch
            df.OHp = 65; df.OWp = 65; df.opad = 2;
            launch_dma(h, conv_gemm_dma_kernel<1, 4, 3, 1, false, true>, df, 96, R[R_IN], S->L[0], R[R_POOL1], 1, ctr + 0);
        } else {
            const int total = batch * C1_TR * C1_TC;
            if (img.f32)
                hipLaunchKernelGGL(conv1_direct_kernel<float>, dim3((unsigned)std::min(total, h->num_cu)), dim3(C1D_THREADS), 0, st, img.f(),
                                   S->mean, S->L[0].wp, S->L[0].bias, R[R_POOL1], 65, 65, 2, ctr + 0, total);
            else
                hipLaunchKernelGGL(conv1_direct_kernel<unsigned char>, dim3((unsigned)std::min(total, h->num_cu)), dim3(C1D_THREADS), 0, st,
                                   img.u8(), S->mean, S->L[0].wp, S->L[0].bias, R[R_POOL1], 65, 65, 2, ctr + 0, total);
        }
        mark();
        mark();
        mark();
    }
    tapunpad(1, R[R_POOL1], 96, 61, 61, 2);
    // conv2 + relu2
    // (a 2-stage / 4-workgroups-per-CU build of the same kernel, NST = 2, WPC = 4, was measured in round 2: conv2 +2 %,
    //  conv3 -3 %, conv5 -11 % (1436 tiles on 1024 workgroups) -- not used)
    // precision 1: the layer's input planes are split into three bf16 NHWC pieces, the GEMM runs on the bf16 matrix cores
    // src_split: the input already is in split format (written by the previous layer); dst_split: write that format
    auto conv_split = [&](int li, const float* src, const unsigned short* src_split, void* dst, bool dst_split) {
        const Layer& l = S->L[li];
        SplitDims sd = l.sd;
        sd.B = batch;
        sd.N = batch * sd.OH * sd.OW;
        const unsigned short* sp = src_split;
        if (!sp) {
            unsigned short* cv = reinterpret_cast<unsigned short*>(R[R_SPLIT]);
            hipLaunchKernelGGL(split_nhwc_kernel, dim3((unsigned)sd.Hp, (unsigned)batch), dim3(256),
                               (size_t)sd.Ctot * (sd.Wp + 1) * sizeof(float), st, src, cv, sd.Ctot, sd.Hp, sd.Wp);
            sp = cv;
        }
        const int ntiles = (sd.N + SG_BN - 1) / SG_BN;
        // measured at B = 102 (ms incl. the split pass): conv2 1.10 / conv3 0.82 with two 4-wave workgroups per CU, 1.21 / 0.90
        // with one 8-wave workgroup; conv5 (718 tiles) 0.53 with 8 waves, 0.62 with 4
        const int variant = S->split_variant == 0 ? (li <= 2 ? 1 : 0) : S->split_variant - 1;
        auto go = [&](auto kernel, int blk, int threads, int per_cu) {
            const int total = sd.groups * ntiles * (sd.mblocks / blk);
            hipLaunchKernelGGL(kernel, dim3((unsigned)std::min(total, per_cu * h->num_cu)), dim3(threads), 0, st, sd, sp, l.wsplit,
                               l.bias, dst, ctr + li, total);
        };
        if (sd.OC == 192) {
            if (dst_split) go(conv_gemm_split_kernel<2, 4, 3, 3, 2, true>, 6, 512, 1);
            else go(conv_gemm_split_kernel<2, 4, 3, 3, 2, false>, 6, 512, 1);
        } else if (variant == 1) {      // two independent 4-wave workgroups per CU, two stages each
            if (dst_split) go(conv_gemm_split_kernel<2, 2, 2, 2, 2, true>, 4, 256, 2);
            else go(conv_gemm_split_kernel<2, 2, 2, 2, 2, false>, 4, 256, 2);
        } else {
            if (dst_split) go(conv_gemm_split_kernel<2, 4, 2, 3, 2, true>, 4, 512, 1);
            else go(conv_gemm_split_kernel<2, 4, 2, 3, 2, false>, 4, 512, 1);
        }
    };
    auto conv_wino = [&](int li, const float* src, float* dst) {      // conv3 / conv4 / conv5 by Winograd F(2 x 2, 3 x 3)
        WinoDims wd = S->L[li].wd;
        wd.tiles = batch * WG_TILES_PER_IMAGE;
        const int total = wd.groups * wd.ocblocks * ((wd.tiles + WG_TB - 1) / WG_TB);
        hipLaunchKernelGGL(conv3x3_winograd_kernel, dim3((unsigned)std::min(total, h->num_cu)), dim3(WG_THREADS), 0, st, wd, src,
                           S->L[li].wino, S->L[li].bias, dst, ctr + li, total, live);
    };
    const bool wino = S->precision == 0 && S->algorithm >= 1;      // Winograd for the layers that are not on pieces
    const bool pieces = S->precision == 0 && S->algorithm >= 2;     // conv2 (mode 3, measurements: conv3 and conv5 too) on exact bf16 pieces
    // conv2..5 as direct convolutions on exact bf16 pieces (cnn_conv_pieces.hpp): the layer's input as P6 planes
    const bool halves = S->precision == 0 && S->algorithm == 4;     // conv2..5 on scaled fp16 pairs (three products per step)
    auto to_p6 = [&](const float* src, unsigned short* dst, int C, int Hp, int Wp, int li) {     // li: the layer that reads the planes
        if (halves) hipLaunchKernelGGL(to_planes_kernel<2>, dim3((unsigned)Hp, (unsigned)(C / 16), (unsigned)batch), dim3(256), 0, st, src, dst, C, Hp, Wp,
                                       S->L[li].ascale, fc.range_word, 1u << li, fc.img_range, live);
        else hipLaunchKernelGGL(to_planes_kernel<3>, dim3((unsigned)Hp, (unsigned)(C / 16), (unsigned)batch), dim3(256), 0, st, src, dst, C, Hp, Wp, 1.f,
                                fc.range_word, 0u, nullptr, live);
    };
    // (planes_next: the next layer's input planes, written by the epilogue instead of the f32 blob -- fp16 pairs only)
    auto conv_pieces = [&](int li, const unsigned short* src6, float* dst, unsigned short* planes_next = nullptr) {
        PieceDims pd = halves ? S->L[li].pdh : S->L[li].pd;
        pd.B = batch;
        if (planes_next) { const PieceDims& nx = S->L[li + 1].pdh; pd.o_cgtot = nx.CGtot; pd.o_Hp = nx.Hp; pd.o_Wp = nx.Wp; pd.o_pad = 1; pd.o_ascale = S->L[li + 1].ascale; }
        pd.range_word = fc.range_word; pd.range_bit = 1u << (li + 1); pd.img_range = fc.img_range; pd.live = live;
        if (halves) pd.oscale = 1.f / (S->L[li].hscale * S->L[li].ascale);
        constexpr int nb = 4;                                               // rows of a wave's four 32 x 32 blocks
        const int tile_rows = halves && li == 3 ? 2 * nb : nb;              // (conv4 on pairs: 64 channels x 8 rows per tile)
        pd.rtiles = (pd.OH + tile_rows - 1) / tile_rows;
        const int total = pd.groups * batch * pd.rtiles * pd.ctiles * pd.mtiles;
        const unsigned blocks = (unsigned)std::min(total, 2 * h->num_cu);   // two workgroups per CU (LDS: two patch buffers each)
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(CP_THREADS), 0, st, pd, src6, halves ? S->L[li].whalf : S->L[li].wsplit, S->L[li].bias,
                               dst, planes_next, ctr + li, total);
        };
        if (halves) { if (li == 1) go(conv_pieces_kernel<5, nb, 2, 1>); else if (li == 3) go(conv_pieces_kernel<3, nb, 2, 2>); else go(conv_pieces_kernel<3, nb, 2, 1>); }
        else { if (li == 1) go(conv_pieces_kernel<5, nb, 3, 1>); else go(conv_pieces_kernel<3, nb, 3, 1>); }
    };
    unsigned short* p6_2 = reinterpret_cast<unsigned short*>(R[R_P6_2]);
    unsigned short* p6_3 = reinterpret_cast<unsigned short*>(R[R_P6_3]);
    unsigned short* p6_5 = reinterpret_cast<unsigned short*>(R[R_P6_5]);
    auto conv_main = [&](int li, const float* src, float* dst) {      // conv2 / conv3 / conv5: 128 x 128 tiles
        if (wino && li >= 2) return conv_wino(li, src, dst);
        if (wino && li == 1) {                                        // conv2 by F(2 x 2, 5 x 5)
            Wino5Dims w5 = S->L[1].wd5;
            w5.tiles = batch * W5_TPI;
            const int total = w5.groups * w5.ocblocks * ((w5.tiles + W5_TB - 1) / W5_TB);
            hipLaunchKernelGGL(conv5x5_winograd_kernel, dim3((unsigned)std::min(total, h->num_cu)), dim3(W5_THREADS), 0, st, w5, src,
                               S->L[1].wino, S->L[1].bias, dst, ctr + 1, total);
            return;
        }
        if (S->precision == 1) return conv_split(li, src, nullptr, dst, false);
        launch_dma(h, conv_gemm_dma_kernel<2, 2, 2, 2, false>, dims(li), 128, src, S->L[li], dst, 1, ctr + li);
    };
    if (pieces) { if (!conv1_hands_planes) to_p6(R[R_POOL1], p6_2, 96, 65, 65, 1); conv_pieces(1, p6_2, R[R_CONV2]); }
    else conv_main(1, R[R_POOL1], R[R_CONV2]);
    mark();
    if ((rc = tapcopy(2, R[R_CONV2], A_CONV2))) return rc;
    // norm2 + pool2 (fused), written with conv3's border
    // (13 rows x 61 columns = 793 pixels per channel and workgroup <= 4 x 256 thread slots; 5 row tiles per image)
    // (13 rows x 61 columns = 793 pixels per channel and workgroup <= 4 x 256 thread slots; 5 row tiles x 8 channel ranges
    //  of 32 channels per image; measured at B = 102: 0.177 ms against 0.235 ms for lrn5_pool3s2_tiled_kernel<6, 15>)
    // fp16 pairs: conv3's input planes straight from the pooling stage (cnn_norm_pool_planes.hpp), unless pool2 is tapped
    const bool hand2 = S->precision == 0 && S->algorithm == 4 && tap != 3;
    if (S->precision == 0 && S->algorithm == 4)
        hipLaunchKernelGGL((lrn5_pool3s2_planes_kernel<6>), dim3((unsigned)(batch * 5 * 8)), dim3(256), 0, st, R[R_CONV2], R[R_POOL2],
                           hand2 ? reinterpret_cast<unsigned short*>(R[R_P6_3]) : nullptr, 256, 61, 61, 30, 30, 1e-4f, 32, 32, 1, 8,
                           S->L[2].ascale, fc.range_word, 1u << 2, fc.img_range);
    else
    hipLaunchKernelGGL((lrn5_pool3s2_stream_kernel<6, 4>), dim3((unsigned)(batch * 5 * 8)), dim3(256), 0, st, R[R_CONV2], R[R_POOL2],
                       256, 61, 61, 30, 30, 1e-4f, 0.75f, 32, 32, 1, 8, live);
    mark();
    mark();
    tapunpad(3, R[R_POOL2], 256, 30, 30, 1);
    // conv3..5.  In split precision conv3 and conv4 hand their result to the next layer in its input format (unless a
    // caller taps the f32 blob)
    const bool chain = S->precision == 1 && tap != 4 && tap != 5;
    unsigned short* s4 = reinterpret_cast<unsigned short*>(R[R_SPLIT4]);
    unsigned short* s5 = reinterpret_cast<unsigned short*>(R[R_SPLIT5]);
    // (pieces: conv3 -> conv4 -> conv5 hand over P6 planes; a tapped f32 blob is converted for the next layer instead)
    // (fp16 pairs: conv3 -> conv4 -> conv5 hand over piece planes -- conv3's epilogue writes conv4's input into p6_5, conv4's writes
    //  conv5's into p6_3, which conv3 has finished reading; a tapped f32 blob is written as such and converted for the next layer)
    const bool hand3 = halves && tap != 4, hand4 = halves && tap != 5;
    if (pieces && S->algorithm >= 3) { if (!hand2) to_p6(R[R_POOL2], p6_3, 256, 32, 32, 2); conv_pieces(2, p6_3, R[R_CONV3], hand3 ? p6_5 : nullptr); }
    else if (chain) conv_split(2, R[R_POOL2], nullptr, s4, true);
    else conv_main(2, R[R_POOL2], R[R_CONV3]);
    mark();
    tapunpad(4, R[R_CONV3], 384, 30, 30, 1);
    if (halves) { if (!hand3) to_p6(R[R_CONV3], p6_5, 384, 32, 32, 3); conv_pieces(3, p6_5, R[R_CONV4], hand4 ? p6_3 : nullptr); }
    else if (chain) conv_split(3, nullptr, s4, s5, true);
    else if (S->precision == 1) conv_split(3, R[R_CONV3], nullptr, R[R_CONV4], false);
    else if (wino) conv_wino(3, R[R_CONV3], R[R_CONV4]);
    else launch_dma(h, conv_gemm_dma_kernel<1, 4, 3, 1, false>, dims(3), 96, R[R_CONV3], S->L[3], R[R_CONV4], 1, ctr + 3);
    mark();
    tapunpad(5, R[R_CONV4], 384, 30, 30, 1);
    if (hand4) conv_pieces(4, p6_3, R[R_CONV5]);
    else if (pieces && S->algorithm >= 3) { to_p6(R[R_CONV4], p6_5, 384, 32, 32, 4); conv_pieces(4, p6_5, R[R_CONV5]); }
    else if (chain) conv_split(4, nullptr, s5, R[R_CONV5], false);
    else conv_main(4, R[R_CONV4], R[R_CONV5]);
    mark();
    if ((rc = tapcopy(6, R[R_CONV5], A_CONV5))) return rc;
    hipLaunchKernelGGL((pool5_kernel<8>), dim3((unsigned)(((long long)batch * 256 + 7) / 8)), dim3(256), 0, st, R[R_CONV5], R[R_POOL5],
                       (long long)batch * 256, live);
    mark();
    if ((rc = tapcopy(7, R[R_POOL5], A_POOL5))) return rc;
    // fc6 / fc7 / fc8: split-K partials + deterministic reduction (+ bias, ReLU / sigmoid)
    float* fc_in = R[R_POOL5];
    float* fc_out = R[R_FCA];
    for (int li = 5; li < 8; ++li) {
        ConvDims d = dims(li);
        if ((li == 5 && pieces) || (halves && li == 6)) {
            // fc6 (fp16 pairs: fc7 too; fc8's 400 outputs are two row tiles: 0.038 ms against 0.030 on the f32 path) on pieces: the input split into B fragments, the weights streamed as f32 in tile order
            // and split in registers (cnn_dense_pieces.hpp): exact bf16 triples, or scaled fp16 pairs under vpk_cnn_set_algorithm(4)
            DenseDims dd;
            dd.N = batch; dd.K = d.K; dd.OC = d.OC; dd.chunks = d.K / DP_CHUNK;
            dd.kparts = li == 5 ? 45 : 16;                        // work items: 16 x 45 / 16 x 16 row tiles x K parts
            dd.cpp = dd.chunks / dd.kparts;
            dd.mtiles = (d.OC + DP_BM - 1) / DP_BM; dd.ntiles = (batch + DP_BN - 1) / DP_BN;
            dd.wscale = halves ? S->L[li].hscale : 1.f;
            dd.live = live;
            dd.oscale = halves ? 1.f / (S->L[li].hscale * S->L[li].ascale) : 1.f;
            const size_t need = (size_t)dd.ntiles * (TOPO[5].IC / DP_CHUNK) * DP_STAGE<3>;
            if ((rc = vpk_reserve(h, (void**)&S->xfrag, &S->xfrag_bytes, need, "hipMalloc(dense input fragments)"))) return rc;
            const int total = dd.mtiles * dd.ntiles * dd.kparts;
            if (halves) {
                hipLaunchKernelGGL(dense_split_kernel<2>, dim3((unsigned)dd.chunks, (unsigned)dd.ntiles), dim3(256), 0, st, fc_in, S->xfrag, batch,
                                   d.K, dd.chunks, S->L[li].ascale, fc.range_word, 1u << li, fc.img_range, nullptr);
                if (S->dense_presplit)
                    hipLaunchKernelGGL(dense_pairs_kernel, dim3((unsigned)std::min(total, h->num_cu)), dim3(DP_THREADS), 0, st, dd, S->L[li].wpair,
                                       S->xfrag, R[R_PART], ctr + li, total);
                else
                hipLaunchKernelGGL(dense_pieces_kernel<2>, dim3((unsigned)std::min(total, h->num_cu)), dim3(DP_THREADS), 0, st, dd, S->L[li].wraw,
                                   S->xfrag, R[R_PART], ctr + li, total);
            } else {
                hipLaunchKernelGGL(dense_split_kernel<3>, dim3((unsigned)dd.chunks, (unsigned)dd.ntiles), dim3(256), 0, st, fc_in, S->xfrag, batch,
                                   d.K, dd.chunks, 1.f, fc.range_word, 0u, nullptr, live);
                hipLaunchKernelGGL(dense_pieces_kernel<3>, dim3((unsigned)std::min(total, h->num_cu)), dim3(DP_THREADS), 0, st, dd, S->L[li].wraw,
                                   S->xfrag, R[R_PART], ctr + li, total);
            }
            d.ksplit = dd.kparts;
        } else
        launch_dma(h, conv_gemm_dma_kernel<2, 2, 2, 2, true>, d, 128, fc_in, S->L[li], R[R_PART], 1, ctr + li, 3, live);
        const long long tot = (long long)d.N * d.OC;
        float* dst = li == 7 ? out : fc_out;
        float* pre = (li == 7 && tap == 10) ? tap_out : nullptr;
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3(ew_blocks(tot)), dim3(256), 0, st, R[R_PART], S->L[li].bias, d.ksplit,
                           d.N, d.OC, li == 7 ? 2 : 1, dst, pre, live);
        mark();
        if (li == 5 && (rc = tapcopy(8, fc_out, A_FC6))) return rc;
        if (li == 6 && (rc = tapcopy(9, fc_out, A_FC7))) return rc;
        fc_in = fc_out;
        fc_out = (li == 5) ? R[R_FCB] : R[R_FCA];
    }
    if (S->profiling) {
        S->ev_valid = (evi == 14);
        if (S->ev_valid) ++S->ev_pass;
    }
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

// ---- activation scales of the fp16-pair layers (cnn_conv_pieces.hpp) ----------------------------------------------------------------
// For each consuming layer (conv2..5, fc6, fc7) the largest |value| of its INPUT blob over a set of calibration rasters, computed by the
// f32 direct kernels -- which do not depend on any scale --, is brought into [32, 64) by a power of two: 2^10 of headroom up to fp16's
// 65 504 for rasters whose activations exceed the calibration set's, and an absolute error floor of 2^-25 / scale (the second piece's
// denormal spacing), i.e. below 2^-30 of the calibration maximum, for rasters whose activations are far below it.
// Built-in calibration set (vpk_cnn_load, vpk_cnn_calibrate(h, NULL, 0)), generated here with integer / single f32 operations only:
//   0  sparse noise: 15 % of the pixels 0..59 (mean 4.4: a raster of a few lines)
//   1  1000 straight strokes blended like sphere_line_plot's curves (alpha 0.1, sphere_mapping.py:62-66): mean ~48, 85 % of the
//      pixels touched, maxima ~240 -- the density of the configs[2..4] rasters (evaluation.py:12-14 with 1000 lines)
//   2  every pixel 255: the largest input the uint8 boundary admits
// The maximum over the set decides: round 5 calibrated on raster 0 alone, and dense rasters spent 3 of its 9 bits of headroom.
// Fixed for the lifetime of the loaded model unless the caller recalibrates: results never depend on earlier forwards.
constexpr int CAL_N = 6;
constexpr int CAL_LAYER[CAL_N] = {1, 2, 3, 4, 5, 6};          // conv2, conv3, conv4, conv5, fc6, fc7
constexpr int CAL_TAP[CAL_N] = {1, 3, 4, 5, 7, 8};            // taps of their inputs: pool1, pool2, conv3, conv4, pool5, fc6
constexpr size_t CAL_SIZE[CAL_N] = {A_POOL1, A_POOL2, A_CONV3, A_CONV4, A_POOL5, A_FC6};
constexpr int CAL_CHUNK = 8;                                   // rasters per calibration forward

// max |x| as the bit pattern of a non-negative float (ordered like unsigned integers; a NaN's pattern is above infinity's)
__global__ void absmax_kernel(const float* __restrict__ x, size_t n, unsigned* __restrict__ out) {
    unsigned m = 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned b = __builtin_bit_cast(unsigned, x[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

void builtin_calibration_rasters(std::vector<uint8_t>& img) {
    const size_t P = 500 * 500;
    img.assign(3 * P, 0);
    unsigned x = 12345u;
    auto next = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (size_t i = 0; i < P; ++i) {
        const unsigned r = next();
        img[i] = (r % 100u) < 15u ? (uint8_t)((r >> 8) % 60u) : 0;
    }
    std::vector<float> canvas(P, 0.f);
    for (int k = 0; k < 1000; ++k) {
        const int y0 = (int)(next() % 500u), y1 = (int)(next() % 500u);
        for (int c = 0; c < 500; ++c) {
            const int y = y0 + ((y1 - y0) * c) / 499;
            float& p = canvas[(size_t)y * 500 + c];
            p = p + 0.1f * (255.f - p);
        }
    }
    for (size_t i = 0; i < P; ++i) img[P + i] = (uint8_t)(canvas[i] + 0.5f);
    for (size_t i = 0; i < P; ++i) img[2 * P + i] = 255;
}

float scale_for_maximum(float m) {
    if (!(m > 0.f) || !std::isfinite(m)) return CP_DEFAULT_ASCALE;
    int ex;
    (void)std::frexp(m, &ex);                  // m = f 2^ex, f in [0.5, 1)
    ex = 6 - ex;                               // m 2^(6 - ex) in [32, 64)
    ex = ex < -100 ? -100 : (ex > 100 ? 100 : ex);
    return std::ldexp(1.f, ex);
}

// the six blob maxima over n rasters on the device
int blob_maxima(vpk_handle* h, const uint8_t* d_imgs, int n, float mx[CAL_N]) {
    vpk_cnn_state* S = h->cnn;
    float *d_out = nullptr, *d_tap = nullptr;
    unsigned* d_max = nullptr;
    auto release = [&]() { (void)hipFree(d_out); (void)hipFree(d_tap); (void)hipFree(d_max); };
    const int chunk = n < CAL_CHUNK ? n : CAL_CHUNK;
    if (hipMalloc((void**)&d_out, (size_t)chunk * 400 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&d_tap, (size_t)chunk * A_POOL1 * sizeof(float)) != hipSuccess ||        // (the largest tapped blob)
        hipMalloc((void**)&d_max, CAL_N * sizeof(unsigned)) != hipSuccess ||
        hipMemsetAsync(d_max, 0, CAL_N * sizeof(unsigned), h->stream) != hipSuccess) {
        release();
        return vpk_fail(h, VPK_ERR_HIP, "vpk_cnn_calibrate: buffers of the calibration forwards");
    }
    const int keep_alg = S->algorithm, keep_fuse = S->fuse_conv1, keep_prec = S->precision;
    const bool keep_prof = S->profiling;
    S->algorithm = 0; S->fuse_conv1 = 1; S->precision = 0; S->profiling = false;
    int rc = VPK_OK;
    for (int b0 = 0; b0 < n && rc == VPK_OK; b0 += chunk) {
        const int nb = n - b0 < chunk ? n - b0 : chunk;
        for (int i = 0; i < CAL_N && rc == VPK_OK; ++i) {
            rc = run_forward(h, Images{d_imgs + (size_t)b0 * 500 * 500, false}, nb, d_out, CAL_TAP[i], d_tap, FwdCtl{S->range_word, nullptr, nullptr});
            if (rc == VPK_OK) hipLaunchKernelGGL(absmax_kernel, dim3(256), dim3(256), 0, h->stream, d_tap, (size_t)nb * CAL_SIZE[i], d_max + i);
        }
    }
    S->algorithm = keep_alg; S->fuse_conv1 = keep_fuse; S->precision = keep_prec; S->profiling = keep_prof;
    unsigned bits[CAL_N] = {};
    if (rc == VPK_OK && (hipStreamSynchronize(h->stream) != hipSuccess ||
                         hipMemcpy(bits, d_max, sizeof(bits), hipMemcpyDeviceToHost) != hipSuccess))
        rc = vpk_fail(h, VPK_ERR_HIP, "vpk_cnn_calibrate: calibration forward failed");
    release();
    for (int i = 0; i < CAL_N; ++i) memcpy(&mx[i], &bits[i], 4);
    return rc;
}

// rasters == nullptr: the built-in set
int calibrate(vpk_handle* h, const uint8_t* rasters, int n) {
    vpk_cnn_state* S = h->cnn;
    uint8_t* d_img = nullptr;
    if (!rasters) {
        std::vector<uint8_t> img;
        builtin_calibration_rasters(img);
        n = (int)(img.size() / (500 * 500));
        if (hipMalloc((void**)&d_img, img.size()) != hipSuccess ||
            hipMemcpy(d_img, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d_img);
            return vpk_fail(h, VPK_ERR_HIP, "vpk_cnn_calibrate: the built-in calibration rasters");
        }
        rasters = d_img;
    }
    float mx[CAL_N];
    const int rc = blob_maxima(h, rasters, n, mx);
    (void)hipFree(d_img);
    if (rc != VPK_OK) return rc;
    for (int i = 0; i < CAL_N; ++i)
        if (!std::isfinite(mx[i]))
            return vpk_fail(h, VPK_ERR_RANGE, "vpk_cnn_calibrate: a blob of the calibration forward is not finite (weights?)");
    for (int i = 0; i < CAL_N; ++i) S->L[CAL_LAYER[i]].ascale = scale_for_maximum(mx[i]);
    return VPK_OK;
}


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
    void* slots = S->act;                                                 // R_IN (region 0): 4 bytes per raster byte (one float image) of room
    float* maps = S->act + off_fca;                                       // R_FCA: 4096 floats per image of room
    hipLaunchKernelGGL(range_compact_kernel, dim3(1), dim3(1024), 0, st, img_range, nb, S->rc_list, S->rc_total);
    if (img.f32)
        hipLaunchKernelGGL(range_gather_kernel<float>, dim3(8, (unsigned)nb), dim3(256), 0, st, img.f(), S->rc_list, static_cast<float*>(slots));
    else
        hipLaunchKernelGGL(range_gather_kernel<uint8_t>, dim3(8, (unsigned)nb), dim3(256), 0, st, img.u8(), S->rc_list, static_cast<uint8_t*>(slots));
    const int keep_alg = S->algorithm, keep_fuse = S->fuse_conv1;
    const bool keep_prof = S->profiling;
    S->algorithm = 2; S->fuse_conv1 = 3; S->profiling = false;
    const int rc = run_forward(h, Images{slots, img.f32}, nb, maps, -1, nullptr, FwdCtl{S->range_word + 1, nullptr, S->rc_list});
    S->algorithm = keep_alg; S->fuse_conv1 = keep_fuse; S->profiling = keep_prof;
    if (rc) return rc;
    hipLaunchKernelGGL(range_scatter_kernel, dim3((unsigned)nb), dim3(128), 0, st, maps, S->rc_list, out);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // namespace

extern "C" {

int vpk_cnn_set_profiling(vpk_handle* h, int on) {
    if (!h || !h->cnn) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_set_profiling before vpk_cnn_load");
    VPK_HIP(h, hipSetDevice(h->device));
    if (on && !h->cnn->ev_ready) {
        for (auto& set : h->cnn->ev)
            for (auto& e : set) VPK_HIP(h, hipEventCreate(&e));
        h->cnn->ev_ready = true;
    }
    h->cnn->profiling = on != 0;
    h->cnn->ev_valid = false;
    h->cnn->ev_pass = 0;
    return VPK_OK;
}

int vpk_cnn_set_fusion(vpk_handle* h, int on) {
    if (!h || !h->cnn) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_set_fusion before vpk_cnn_load");
    h->cnn->fuse_conv1 = on < 0 ? 0 : (on > 4 ? 4 : on);
    return VPK_OK;
}

#ifdef W5_TIME
int vpk_dbg_w5(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(w5_dbg), sizeof(long long) * 256 * 12 * 8); }
int vpk_dbg_w3(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(w3_dbg), sizeof(long long) * 256 * 8 * 8); }
#endif

int vpk_cnn_set_algorithm(vpk_handle* h, int mode) {
    if (!h || !h->cnn) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_set_algorithm before vpk_cnn_load");
    if (mode < 0 || mode > 4) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_set_algorithm: mode must be 0 .. 4");
    h->cnn->algorithm = mode;
    return VPK_OK;
}

int vpk_cnn_set_precision(vpk_handle* h, int mode) {
    if (!h || !h->cnn) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_set_precision before vpk_cnn_load");
    if (mode < 0 || mode > 3) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_set_precision: mode must be 0 or 1");
    h->cnn->precision = mode ? 1 : 0;
    h->cnn->split_variant = mode > 1 ? mode - 1 : 0;   // 2, 3: force one tiling for every layer (development)
    return VPK_OK;
}

int vpk_cnn_last_layer_ms(vpk_handle* h, float ms[13]) {
    if (!h || !ms || !h->cnn) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_last_layer_ms: bad argument");
    if (!h->cnn->ev_valid) return vpk_fail(h, VPK_ERR_STATE, "no profiled forward pass recorded");
    hipEvent_t* evs = h->cnn->ev[(h->cnn->ev_pass - 1) % vpk_cnn_state::EV_RING];
    VPK_HIP(h, hipEventSynchronize(evs[13]));
    for (int i = 0; i < 13; ++i) VPK_HIP(h, hipEventElapsedTime(&ms[i], evs[i], evs[i + 1]));
    return VPK_OK;
}

int vpk_cnn_mean_layer_ms(vpk_handle* h, float ms[13], int* passes) {
    if (!h || !ms || !h->cnn) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_mean_layer_ms: bad argument");
    vpk_cnn_state* S = h->cnn;
    if (!S->ev_valid || S->ev_pass < 1) return vpk_fail(h, VPK_ERR_STATE, "no profiled forward pass recorded");
    const long long n = S->ev_pass < vpk_cnn_state::EV_RING ? S->ev_pass : vpk_cnn_state::EV_RING;
    double sum[13] = {};
    for (long long q = S->ev_pass - n; q < S->ev_pass; ++q) {
        hipEvent_t* evs = S->ev[q % vpk_cnn_state::EV_RING];
        VPK_HIP(h, hipEventSynchronize(evs[13]));
        for (int i = 0; i < 13; ++i) {
            float t = 0.f;
            VPK_HIP(h, hipEventElapsedTime(&t, evs[i], evs[i + 1]));
            sum[i] += t;
        }
    }
    for (int i = 0; i < 13; ++i) ms[i] = (float)(sum[i] / (double)n);
    if (passes) *passes = (int)n;
    return VPK_OK;
}

int vpk_cnn_load(vpk_handle* h, const float* const blobs[16], const float* mean) {
    if (!h || !blobs || !mean) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_load: null argument");
    for (int i = 0; i < 16; ++i)
        if (!blobs[i]) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_load: null blob");
    VPK_HIP(h, hipSetDevice(h->device));
    vpk_cnn_free(h);
    h->cnn = new vpk_cnn_state();
    vpk_cnn_state* S = h->cnn;
    VPK_HIP(h, hipMalloc((void**)&S->mean, 500 * 500 * sizeof(float)));
    VPK_HIP(h, hipMemcpy(S->mean, mean, 500 * 500 * sizeof(float), hipMemcpyHostToDevice));
    for (int li = 0; li < 8; ++li) {
        const Topo& t = TOPO[li];
        Layer& l = S->L[li];
        ConvDims& d = l.d;
        d.B = 0; d.IC = t.IC; d.Hp = t.H + 2 * t.P; d.Wp = t.W + 2 * t.P; d.OC = t.OC; d.OH = t.OH; d.OW = t.OW; d.groups = t.G;
        d.OHp = t.OH + 2 * t.OP; d.OWp = t.OW + 2 * t.OP; d.opad = t.OP;
        if (li == 0) { d.IC = C1_PH * C1_PH; d.Hp = C1_PW; d.Wp = C1_PW; }   // phase planes (K stays 11 x 11)
        d.K = t.IC * t.KH * t.KH;
        d.Kp = (d.K + BK - 1) / BK * BK;
        d.Mp = (t.OC + t.BM - 1) / t.BM * t.BM;
        d.N = 0;
        d.ksplit = KSPLIT[li];
        d.relu = 1;
        const size_t w_floats = (size_t)t.G * t.OC * d.K;
        const size_t p_floats = (size_t)t.G * d.Kp * d.Mp;
        float* raw = nullptr;
        VPK_HIP(h, hipMalloc((void**)&raw, w_floats * sizeof(float)));
        VPK_HIP(h, hipMemcpy(raw, blobs[2 * li], w_floats * sizeof(float), hipMemcpyHostToDevice));
        VPK_HIP(h, hipMalloc((void**)&l.wp, p_floats * sizeof(float)));
        hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((p_floats + 255) / 256)), dim3(256), 0, h->stream, raw,
                           l.wp, t.G, t.OC, d.K, d.Kp, d.Mp);
        VPK_HIP(h, hipStreamSynchronize(h->stream));
        if (li == 5 || li == 6) {       // fc6, fc7: also as f32 in tile order for the pieces path (cnn_dense_pieces.hpp)
            const int chunks = d.K / DP_CHUNK, mtiles = (t.OC + DP_BM - 1) / DP_BM;
            const long long total4 = (long long)mtiles * chunks * DP_BM * (DP_CHUNK / 4);
            VPK_HIP(h, hipMalloc((void**)&l.wraw, (size_t)total4 * 16));
            hipLaunchKernelGGL(dense_tile_weights_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, h->stream, raw, l.wraw, t.OC, d.K,
                               chunks, total4);
            VPK_HIP(h, hipStreamSynchronize(h->stream));
            float wmax = 0.f;
            for (size_t i = 0; i < w_floats; ++i) wmax = std::max(wmax, std::fabs(blobs[2 * li][i]));
            int ex = 0;
            if (wmax > 0.f) (void)std::frexp(wmax, &ex);
            l.hscale = std::ldexp(1.f, wmax > 0.f ? 14 - ex : 0);
            // ... and as scaled fp16 pairs in the A-fragment order of dense_pairs_kernel (4 bytes per weight, like the f32 copy)
            const long long total16 = (long long)mtiles * chunks * 8 * 2 * 2 * 64;
            VPK_HIP(h, hipMalloc((void**)&l.wpair, (size_t)total16 * 16));
            hipLaunchKernelGGL(dense_pair_weights_kernel, dim3((unsigned)((total16 + 255) / 256)), dim3(256), 0, h->stream, raw, l.wpair, t.OC,
                               d.K, chunks, l.hscale, total16);
            VPK_HIP(h, hipStreamSynchronize(h->stream));
            VPK_HIP(h, hipFree(raw));
        }
        else VPK_HIP(h, hipFree(raw));
        if (li < 5) {   // convolution: byte offset of tap k from the patch origin, in the bordered planes;
                        // the K padding (conv1: 121 -> 128) points at offset 0 and meets zero weights
            std::vector<unsigned> tab(d.Kp, 0u);
            for (int k = 0; k < d.K; ++k) {
                int ic = k / (t.KH * t.KH), r = k % (t.KH * t.KH), kh = r / t.KH, kw = r % t.KH;
                if (li == 0)   // conv1 reads the stride-4 phase planes written by prep_input_kernel
                    tab[k] = (unsigned)((((kh % C1_PH) * C1_PH + kw % C1_PH) * C1_PW + kh / C1_PH) * C1_PW + kw / C1_PH) * 4u;
                else
                    tab[k] = (unsigned)((ic * d.Hp + kh) * d.Wp + kw) * 4u;
            }
            VPK_HIP(h, hipMalloc((void**)&l.ktab, tab.size() * sizeof(unsigned)));
            VPK_HIP(h, hipMemcpy(l.ktab, tab.data(), tab.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        }
        if (li >= 1 && li <= 4) {   // three bf16 pieces of every weight, in the A-fragment order of v_mfma_f32_32x32x16_bf16
            SplitDims& sd = l.sd;
            const int blk = t.OC == 192 ? 6 : 4;                      // 32-row blocks per tile
            sd.B = 0; sd.Cg = t.IC; sd.Ctot = t.IC * t.G; sd.Hp = d.Hp; sd.Wp = d.Wp; sd.OC = t.OC; sd.OH = t.OH; sd.OW = t.OW;
            sd.groups = t.G; sd.KW = t.KH; sd.ntaps = t.KH * t.KH; sd.csteps = t.IC / 16; sd.ksteps = sd.ntaps * sd.csteps;
            sd.mblocks = (t.OC / 32 + blk - 1) / blk * blk; sd.N = 0; sd.relu = 1; sd.OHp = d.OHp; sd.OWp = d.OWp; sd.opad = d.opad;
            const size_t frag = (size_t)t.G * sd.ksteps * sd.mblocks * 3;
            std::vector<unsigned short> pk(frag * 512, 0);
            const float* wsrc = blobs[2 * li];
            for (int g = 0; g < t.G; ++g)
                for (int s_ = 0; s_ < sd.ksteps; ++s_)
                    for (int mb = 0; mb < sd.mblocks; ++mb)
                        for (int ln = 0; ln < 64; ++ln)
                            for (int e = 0; e < 8; ++e) {
                                const int m = mb * 32 + (ln & 31);
                                const int tap = s_ % sd.ntaps, c = (s_ / sd.ntaps) * 16 + 8 * (ln >> 5) + e;   // step = (channel group, tap)
                                float w = 0.f;
                                if (m < t.OC) w = wsrc[((size_t)(g * t.OC + m) * t.IC + c) * t.KH * t.KH + tap];
                                auto rne = [](float x) { unsigned b; memcpy(&b, &x, 4); return (b + 0x7fffu + ((b >> 16) & 1u)) & 0xffff0000u; };
                                const unsigned b0 = rne(w);                 // the same three pieces as split3() on the device
                                float f0; memcpy(&f0, &b0, 4);
                                const float r1 = w - f0;
                                const unsigned b1 = rne(r1);
                                float f1; memcpy(&f1, &b1, 4);
                                const float r2 = r1 - f1;
                                unsigned b2; memcpy(&b2, &r2, 4);
                                const size_t base = ((((size_t)g * sd.ksteps + s_) * sd.mblocks + mb) * 3) * 512 + (size_t)ln * 8 + e;
                                pk[base] = (unsigned short)(b0 >> 16);
                                pk[base + 512] = (unsigned short)(b1 >> 16);
                                pk[base + 1024] = (unsigned short)(b2 >> 16);
                            }
            VPK_HIP(h, hipMalloc((void**)&l.wsplit, pk.size() * sizeof(unsigned short)));
            VPK_HIP(h, hipMemcpy(l.wsplit, pk.data(), pk.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
            PieceDims& pd = l.pd;                                     // the same fragments feed conv_pieces_kernel
            pd.B = 0; pd.Cg16 = t.IC / 16; pd.CGtot = t.IC * t.G / 16; pd.Hp = d.Hp; pd.Wp = d.Wp; pd.OC = t.OC; pd.OH = t.OH; pd.OW = t.OW;
            pd.groups = t.G; pd.KW = t.KH; pd.ntaps = t.KH * t.KH; pd.ksteps = sd.ksteps; pd.mblocks = sd.mblocks;
            pd.mtiles = sd.mblocks / blk; pd.rtiles = (t.OH + 3) / 4; pd.ctiles = (t.OW + CP_TC - 1) / CP_TC; pd.relu = 1;
            pd.OHp = d.OHp; pd.OWp = d.OWp; pd.opad = d.opad;
            pd.in_image = (long long)pd.CGtot * 6 * d.Hp * d.Wp * 16;
            pd.oscale = 1.f;
            // the same layer on fp16 pairs: weights x 2^k (the largest in [2^13, 2^14)), two pieces each; 32-row blocks padded to
            // whole tiles (none needed: 4 per tile, conv4 2)
            PieceDims& ph = l.pdh;
            ph = pd;
            const int mbt = li == 3 ? 2 : 4;                          // 32-row blocks per tile: 128 channels x 4 rows; conv4 (192 channels per group) 64 x 8
            ph.mblocks = (t.OC / 32 + mbt - 1) / mbt * mbt;
            ph.mtiles = ph.mblocks / mbt;
            ph.in_image = (long long)ph.CGtot * 4 * d.Hp * d.Wp * 16;
            float wmax = 0.f;
            for (size_t i = 0; i < w_floats; ++i) wmax = std::max(wmax, std::fabs(wsrc[i]));
            int kexp = 0;
            if (wmax > 0.f) { int ex; (void)std::frexp(wmax, &ex); kexp = 14 - ex; }     // wmax = f * 2^ex, f in [0.5, 1): wmax * 2^kexp in [2^13, 2^14)
            const float wscale = std::ldexp(1.f, kexp);
            l.hscale = wscale;
            ph.oscale = 1.f / (wscale * l.ascale);               // (set again per forward: the activation scale is calibrated after the load)
            std::vector<unsigned short> ph_pk((size_t)t.G * ph.ksteps * ph.mblocks * 2 * 512, 0);
            for (int g = 0; g < t.G; ++g)
                for (int s_ = 0; s_ < ph.ksteps; ++s_)
                    for (int mb = 0; mb < ph.mblocks; ++mb)
                        for (int ln = 0; ln < 64; ++ln)
                            for (int e = 0; e < 8; ++e) {
                                const int m = mb * 32 + (ln & 31);
                                const int tap = s_ % ph.ntaps, c = (s_ / ph.ntaps) * 16 + 8 * (ln >> 5) + e;
                                float w = 0.f;
                                if (m < t.OC) w = wsrc[((size_t)(g * t.OC + m) * t.IC + c) * t.KH * t.KH + tap] * wscale;
                                const _Float16 h0 = (_Float16)w;
                                const _Float16 h1 = (_Float16)(w - (float)h0);
                                unsigned short u0, u1;
                                memcpy(&u0, &h0, 2); memcpy(&u1, &h1, 2);
                                const size_t base = ((((size_t)g * ph.ksteps + s_) * ph.mblocks + mb) * 2) * 512 + (size_t)ln * 8 + e;
                                ph_pk[base] = u0;
                                ph_pk[base + 512] = u1;
                            }
            VPK_HIP(h, hipMalloc((void**)&l.whalf, ph_pk.size() * sizeof(unsigned short)));
            VPK_HIP(h, hipMemcpy(l.whalf, ph_pk.data(), ph_pk.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
        }
        if (li == 0) {              // conv1 on the bf16 matrix cores: weight pieces in fragment order, bias - conv1(mean)
            std::vector<unsigned short> fr;
            conv1_pieces_weights(blobs[0], fr);
            VPK_HIP(h, hipMalloc((void**)&l.c1frag, fr.size() * sizeof(unsigned short)));
            VPK_HIP(h, hipMemcpy(l.c1frag, fr.data(), fr.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
            {
                float wmax = 0.f;
                for (int i = 0; i < 96 * 121; ++i) wmax = std::max(wmax, std::fabs(blobs[0][i]));
                int ex = 0;
                if (wmax > 0.f) (void)std::frexp(wmax, &ex);
                l.c1scale = std::ldexp(1.f, wmax > 0.f ? 14 - ex : 0);
                conv1_pieces_weights(blobs[0], fr, 2, l.c1scale);
                VPK_HIP(h, hipMalloc((void**)&l.c1half, fr.size() * sizeof(unsigned short)));
                VPK_HIP(h, hipMemcpy(l.c1half, fr.data(), fr.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
            }
            std::vector<float> cm;
            conv1_pieces_cmap(blobs[0], blobs[1], mean, cm);
            VPK_HIP(h, hipMalloc((void**)&l.c1map, cm.size() * sizeof(float)));
            VPK_HIP(h, hipMemcpy(l.c1map, cm.data(), cm.size() * sizeof(float), hipMemcpyHostToDevice));
            if (const char* e = getenv("VPK_CONV1_GROUP")) { const int v = atoi(e); if (v >= 1 && v <= 64) S->conv1_group = v; }
            if (const char* e = getenv("VPK_DENSE_PRESPLIT")) S->dense_presplit = atoi(e) != 0;
        }
        if (li == 1) {              // conv2: G g G^T of every 5 x 5 filter (F(2 x 2, 5 x 5))
            std::vector<float> u;
            winograd5_weights(blobs[2], t.G, t.OC, t.IC, u);
            VPK_HIP(h, hipMalloc((void**)&l.wino, u.size() * sizeof(float)));
            VPK_HIP(h, hipMemcpy(l.wino, u.data(), u.size() * sizeof(float), hipMemcpyHostToDevice));
            Wino5Dims& w5 = l.wd5;
            w5.IC = t.IC; w5.OC = t.OC; w5.groups = t.G; w5.ctot_in = t.IC * t.G; w5.ctot_out = t.OC * t.G; w5.tiles = 0;
            w5.ocblocks = t.OC / W5_OCB; w5.chunks = t.IC / W5_KC; w5.relu = 1;
        }
        if (li >= 2 && li <= 4) {   // G g G^T of every 3 x 3 filter, in the order conv3x3_winograd_kernel streams it
            std::vector<float> u;
            winograd_weights(blobs[2 * li], t.G, t.OC, t.IC, u);
            VPK_HIP(h, hipMalloc((void**)&l.wino, u.size() * sizeof(float)));
            VPK_HIP(h, hipMemcpy(l.wino, u.data(), u.size() * sizeof(float), hipMemcpyHostToDevice));
            WinoDims& wd = l.wd;
            wd.IC = t.IC; wd.OC = t.OC; wd.groups = t.G; wd.ctot_in = t.IC * t.G; wd.ctot_out = t.OC * t.G; wd.tiles = 0;
            wd.ocblocks = t.OC / WG_OCB; wd.chunks = t.IC / WG_KC; wd.OHp = d.OHp; wd.OWp = d.OWp; wd.opad = d.opad; wd.relu = 1;
        }
        VPK_HIP(h, hipMalloc((void**)&l.bias, (size_t)t.G * t.OC * sizeof(float)));
        VPK_HIP(h, hipMemcpy(l.bias, blobs[2 * li + 1], (size_t)t.G * t.OC * sizeof(float), hipMemcpyHostToDevice));
    }
    VPK_HIP(h, hipMalloc((void**)&S->range_word, 256));
    VPK_HIP(h, hipMemset(S->range_word, 0, 256));
    VPK_HIP(h, hipMalloc((void**)&S->rc_list, (1 + MAX_CHUNK) * sizeof(int)));
    VPK_HIP(h, hipMalloc((void**)&S->rc_total, sizeof(unsigned long long)));
    VPK_HIP(h, hipMemset(S->rc_total, 0, sizeof(unsigned long long)));
    // the activation scales of the fp16-pair layers: six tapped forwards of the built-in calibration rasters on the f32 direct
    // kernels (calibrate()); their arena (batch 3) is released again so that the first real forward allocates once, for its batch
    const int rc = calibrate(h, nullptr, 0);
    if (S->act) { (void)hipFree(S->act); S->act = nullptr; S->act_bytes = 0; S->act_batch = 0; }
    if (rc != VPK_OK) return rc;                // (the model stays unloaded: vpk_cnn_forward refuses)
    S->loaded = true;
    return VPK_OK;
}

int vpk_cnn_calibrate(vpk_handle* h, const uint8_t* rasters, int n) {
    if (!h || n < 0 || (n > 0 && !rasters)) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_calibrate: bad argument");
    if (!h->cnn || !h->cnn->loaded) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_calibrate before vpk_cnn_load");
    if (n > 0 && ((size_t)rasters & 3) != 0) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_calibrate: the rasters must be 4-byte aligned");
    VPK_HIP(h, hipSetDevice(h->device));
    return calibrate(h, n > 0 ? rasters : nullptr, n);
}

int vpk_cnn_get_activation_scales(vpk_handle* h, float scales[6]) {
    if (!h || !scales) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_get_activation_scales: null argument");
    if (!h->cnn || !h->cnn->loaded) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_get_activation_scales before vpk_cnn_load");
    for (int i = 0; i < CAL_N; ++i) scales[i] = h->cnn->L[CAL_LAYER[i]].ascale;
    return VPK_OK;
}

int vpk_cnn_set_activation_scales(vpk_handle* h, const float scales[6]) {
    if (!h || !scales) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_set_activation_scales: null argument");
    if (!h->cnn || !h->cnn->loaded) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_set_activation_scales before vpk_cnn_load");
    for (int i = 0; i < CAL_N; ++i) {
        int ex = 0;
        const float f = std::frexp(scales[i], &ex);
        if (!(scales[i] > 0.f) || !std::isfinite(scales[i]) || f != 0.5f || ex < -99 || ex > 101)
            return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_set_activation_scales: every scale must be a power of two in 2^-100 .. 2^100");
    }
    for (int i = 0; i < CAL_N; ++i) h->cnn->L[CAL_LAYER[i]].ascale = scales[i];
    return VPK_OK;
}

int vpk_cnn_range_flags(vpk_handle* h, uint32_t* flags_out) {
    if (!h) return VPK_ERR_ARG;
    if (!h->cnn || !h->cnn->loaded) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_range_flags before vpk_cnn_load");
    VPK_HIP(h, hipSetDevice(h->device));
    unsigned word = 0;
    VPK_HIP(h, hipMemcpyAsync(&word, h->cnn->range_word, sizeof(word), hipMemcpyDeviceToHost, h->stream));
    VPK_HIP(h, hipMemsetAsync(h->cnn->range_word, 0, sizeof(word), h->stream));
    VPK_HIP(h, hipStreamSynchronize(h->stream));
    if (flags_out) *flags_out = word;
    if (!word) return VPK_OK;
    static const char* names[8] = {"", "conv2", "conv3", "conv4", "conv5", "fc6", "fc7", ""};
    std::string msg = "vpk_cnn_forward: scaled fp16-pair activations reached fp16's range (clamped to 65504) at the input of";
    for (int li = 1; li <= 6; ++li)
        if (word & (1u << li)) msg += std::string(" ") + names[li];
    msg += ": the response maps of the forwards since the last check are NOT the net's; recalibrate (vpk_cnn_calibrate) or use vpk_cnn_set_algorithm(2)";
    return vpk_fail(h, VPK_ERR_RANGE, msg.c_str());
}

}  // extern "C"

namespace {
// policy: vpk_cnn_forward (per-image flags kept, the range policy applied); !policy: vpk_cnn_forward_tap, as before the policy existed
int forward_chunks(vpk_handle* h, Images sphere, int batch, float* out, int tap, float* tap_out, bool policy) {
    if (!h || !sphere.p || !out || batch < 1) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_forward: bad argument");
    if (!sphere.f32 && ((size_t)sphere.p & 3) != 0)      // conv1's loader reads four horizontally adjacent pixels as one 4-byte word
        return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_forward: the rasters must be 4-byte aligned");
    if (sphere.f32 && ((size_t)sphere.p & 15) != 0)      // ... as one 16-byte word
        return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_forward_f32: the images must be 16-byte aligned");
    if (!h->cnn || !h->cnn->loaded) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_forward before vpk_cnn_load");
    VPK_HIP(h, hipSetDevice(h->device));
    // activations for the whole batch stay in HBM; chunk only if they would exceed a third of it
    // (and at 4096 images: positions and dense-layer byte offsets are 32-bit inside one launch)
    const size_t per_img = arena_floats_per_image() * sizeof(float);
    int chunk = (int)std::min<size_t>(std::min<size_t>((size_t)batch, MAX_CHUNK),
                                      std::max<size_t>(1, (h->total_mem / 3) / per_img));
    static const size_t tap_size[11] = {A_CONV1, A_POOL1, A_CONV2, A_POOL2, A_CONV3, A_CONV4, A_CONV5, A_POOL5,
                                        A_FC6, A_FC7, A_FC8};
    vpk_cnn_state* S = h->cnn;
    if (policy) {
        int rc = vpk_reserve(h, (void**)&S->img_range, &S->img_range_bytes, (size_t)batch * sizeof(unsigned), "hipMalloc(per-image range flags)");
        if (rc) return rc;
        VPK_HIP(h, hipMemsetAsync(S->img_range, 0, (size_t)batch * sizeof(unsigned), h->stream));
        S->img_range_batch = batch;
    }
    // only the fp16-pair configuration can clamp: the recompute pass is not even launched for the others
    const bool recompute = policy && S->range_policy == 1 && S->precision == 0 && S->algorithm == 4;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        int nb = std::min(chunk, batch - b0);
        float* tp = (tap_out && tap >= 0 && tap <= 10) ? tap_out + (size_t)b0 * tap_size[tap] : nullptr;
        const Images sp = sphere.at((size_t)b0);
        float* op = out + (size_t)b0 * 400;
        unsigned* img = policy ? S->img_range + b0 : nullptr;
        int rc = run_forward(h, sp, nb, op, tp ? tap : -1, tp, FwdCtl{recompute ? S->range_word + 1 : S->range_word, img, nullptr});
        if (!rc && recompute) rc = recompute_flagged(h, sp, nb, op, img);
        if (rc) return rc;
    }
    return VPK_OK;
}
}  // namespace

extern "C" {

int vpk_cnn_forward_tap(vpk_handle* h, const uint8_t* sphere, int batch, float* out, int tap, float* tap_out) {
    return forward_chunks(h, Images{sphere, false}, batch, out, tap, tap_out, false);
}

int vpk_cnn_forward(vpk_handle* h, const uint8_t* sphere, int batch, float* out) {
    return forward_chunks(h, Images{sphere, false}, batch, out, -1, nullptr, true);
}

int vpk_cnn_forward_tap_f32(vpk_handle* h, const float* image, int batch, float* out, int tap, float* tap_out) {
    return forward_chunks(h, Images{image, true}, batch, out, tap, tap_out, false);
}

int vpk_cnn_forward_f32(vpk_handle* h, const float* image, int batch, float* out) {
    return forward_chunks(h, Images{image, true}, batch, out, -1, nullptr, true);
}

int vpk_cnn_set_range_policy(vpk_handle* h, int policy) {
    if (!h || !h->cnn) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_set_range_policy before vpk_cnn_load");
    if (policy != 0 && policy != 1) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_set_range_policy: policy must be 0 (RAISE) or 1 (RECOMPUTE_EXACT)");
    h->cnn->range_policy = policy;
    return VPK_OK;
}

int vpk_cnn_image_range_flags(vpk_handle* h, int batch, uint32_t* flags_out) {
    if (!h || !flags_out || batch < 1) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_image_range_flags: bad argument");
    if (!h->cnn || !h->cnn->loaded) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_image_range_flags before vpk_cnn_load");
    if (h->cnn->img_range_batch == 0) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_image_range_flags before any vpk_cnn_forward");
    if (batch != h->cnn->img_range_batch)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_image_range_flags: batch differs from the last vpk_cnn_forward's");
    VPK_HIP(h, hipSetDevice(h->device));
    VPK_HIP(h, hipMemcpyAsync(flags_out, h->cnn->img_range, (size_t)batch * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    VPK_HIP(h, hipStreamSynchronize(h->stream));
    return VPK_OK;
}

int vpk_cnn_recomputed(vpk_handle* h, int64_t* n_out) {
    if (!h || !n_out) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_recomputed: null argument");
    if (!h->cnn || !h->cnn->loaded) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_recomputed before vpk_cnn_load");
    VPK_HIP(h, hipSetDevice(h->device));
    unsigned long long n = 0;
    VPK_HIP(h, hipMemcpyAsync(&n, h->cnn->rc_total, sizeof(n), hipMemcpyDeviceToHost, h->stream));
    VPK_HIP(h, hipMemsetAsync(h->cnn->rc_total, 0, sizeof(n), h->stream));
    VPK_HIP(h, hipStreamSynchronize(h->stream));
    *n_out = (int64_t)n;
    return VPK_OK;
}

}  // extern "C"
