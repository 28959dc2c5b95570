// cnn_conv1_direct.hpp -- conv1 + relu1 + norm1 + pool1 as one direct f32 convolution (vpk_cnn_set_fusion(1)): the kernel
// calibration and the accuracy rule run on.  Included by vpk_cnn.hip after cnn_gemm_f32.hpp (the C1_* patch constants).
// -DC1D_TIME: per-phase clocks of the kernel (scripts/c1d_phase_times.py).
#ifndef VPK_CNN_CONV1_DIRECT_HPP_
#define VPK_CNN_CONV1_DIRECT_HPP_

#include <type_traits>

#include "cnn_prims.hpp"   // f32x2, f32x4, lds_barrier, TileQueue

namespace {

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

// (the barriers are lds_barrier(), cnn_prims.hpp: the pooled outputs' global stores stay in flight across them, where
//  __syncthreads would wait for one HBM write round trip per tile)

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
    TileQueue queue{s_next};
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
    // The tile queue (cnn_prims.hpp) TWO tiles ahead: `next`'s patch is loaded under `tile`'s MFMAs, so the index of the tile after
    // next is what a tile fetches -- the compiler's atomicAdd at its top, consumed (stored, read back) only at its end, so that the
    // atomic's round trip is never waited for.  The slots alternate with the iteration, not with a parity of the queue's.
    int tile = blockIdx.x;
    f32x4 pre[PRE];
    Raw pre8[PRE];
    if (tile < total_tiles) { patch_load(tile, pre, pre8); patch_store(pre, pre8); }
    queue.take(tile_counter, 0);
    __syncthreads();
    int next = queue.peek(0);
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
        next = queue.peek((it + 1) & 1);
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

}  // namespace
#endif
