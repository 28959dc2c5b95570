// cnn_gemm_f32.hpp -- the f32 implicit-GEMM path of every conv / dense layer on the exact-f32 matrix cores
// (v_mfma_f32_32x32x2_f32): conv_gemm_dma_kernel, the split-K reduction of the dense layers and the load-time weight
// re-pack into k-major panels.  Included by vpk_cnn.hip.
#ifndef VPK_CNN_GEMM_F32_HPP_
#define VPK_CNN_GEMM_F32_HPP_

#include "cnn_model.hpp"   // ConvDims, BK, C1_*
#include "cnn_prims.hpp"   // f32x16, LDS-DMA, waits, TileQueue

namespace {

constexpr int CONV_THREADS = 256;

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
// (lds_dma16 / lds_dma4, wait_vmcnt, lds_barrier and the tile queue: cnn_prims.hpp, which also says why they are inline asm;
//  completion of a stage's DMA is counted by wait_stage below)

// conv1 + norm1 + pool1 as ONE kernel (C1FUSE): a tile's 128 columns are a 2-D patch of 7 x 17 conv1 outputs
// (all 96 channels: one M tile, so the LRN across channels is local to the tile); after the K loop the patch
// goes to LDS (over the then idle stage buffers), is normalised in place and max-pooled to 3 x 8 outputs per
// channel, and only those are written -- conv1's 0.59 GB output (B = 102) never exists.  Neighbouring patches
// share one conv row / column (pooling windows overlap by one), i.e. 7/6 x 17/16 = 1.24x the MFMA work.
// (the patch constants C1_*: cnn_model.hpp)

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
    __shared__ int s_next[2];
    TileQueue queue{s_next};                            // persistent workgroups over the layer's tiles (cnn_prims.hpp)
    if (!C1FUSE && live) {                              // recompute pass (vpk_cnn_set_range_policy): the device count's images only
        d.B = __builtin_amdgcn_readfirstlane(*live);
        d.N = d.B * d.OH * d.OW;
        total_tiles = d.groups * d.ksplit * ((d.N + BN - 1) / BN) * (d.Mp / BM);
    }
    for (int tile = blockIdx.x; tile < total_tiles;) {
    int nx = queue.request(tile_counter);               // the oldest vector-memory op of wave 0: complete at the first wait_stage
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
    const unsigned as_base = lds_addr_of(&As[0][0][0]), bs_base = lds_addr_of(&Bs[0][0][0]);
    auto issue = [&](int kt, int buf) {
        const int k0 = kt * BK;
        const float* abase = wpan + (size_t)k0 * d.Mp;
#pragma unroll
        for (int r = 0; r < A_IT; ++r) {
            const int idx0 = r * CONV_THREADS + wave * 64;         // wave-uniform first float4 of this piece
            if (idx0 < A_F4)
                lds_dma16(aoff[r], abase, __builtin_amdgcn_readfirstlane(as_base + (unsigned)((buf * BK * BM + idx0 * 4) * 4)));
        }
        if (DENSE) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {                            // this wave's two k quads (of four), its half of the columns
                const int kq = (wave >> 1) * 2 + q;
                lds_dma16(boff, bbase + k0 + 4 * kq, __builtin_amdgcn_readfirstlane(
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
            lds_dma4(boff, (const char*)bbase + e[q], __builtin_amdgcn_readfirstlane(
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
    queue.publish(nx);
    lds_barrier();
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
        lds_barrier();                                  // ... for every wave; stage t's buffer is free again
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
    tile = queue.next();
    }   // tile loop
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

}  // namespace
#endif
