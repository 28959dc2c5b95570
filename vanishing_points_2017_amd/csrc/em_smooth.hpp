// em_smooth.hpp -- the smoothers (weight_matrix, the (M x N) . (N x N) product): round-1/2 kernels, the row-sliced kernel, the sparse
// one, and the dispatch between them.
// One part of em_device.hpp (the conventions, and why the unit is compiled with -ffp-contract=off, are there).
#ifndef VPK_EM_SMOOTH_HPP_
#define VPK_EM_SMOOTH_HPP_

#include "em_ctx.hpp"
#include "em_estep.hpp"

namespace vpk {

// ---------------------------------------------------------------------------------------------
// smoothing: weight_matrix (vp_localisation.py:515-524), the (M x N) . (N x N) product
// ---------------------------------------------------------------------------------------------
// w[m][k] = (w_[m][k] + bias*lweight[k] * sum_j w_[m][j] lsim[j][k]) / den[k].
// Work decomposition: an output block = (64*C consecutive columns) x (MT VPs); every wave owns
// whole blocks and walks ALL rows j for them, so no cross-wave reduction is needed and the result
// is deterministic.  A lane holds C adjacent columns (C = 2: one 16-byte load per row, a wave reads
// 1 KiB of contiguous lsim per row) and MT accumulators per column; rows are unrolled UNR deep so
// UNR independent loads are in flight per lane (HBM latency is hidden by bytes in flight, not by
// occupancy).  The w_ operand (wsrc[j][m]) is staged through LDS in row chunks and read as a
// wave-uniform broadcast.
template <int C, int UNR>
VPK_DEVFN void smooth_blocks(EmCtx& c) {
    Shared& sh = SH();
    const int M = sh.M, N = c.N;
    const int colw = WAVE * C;
    const int ncg = (N + colw - 1) / colw;
    const int ntile = (M + MT - 1) / MT;
    const int W = ntile * MT;                       // staged VPs per row (<= mcap)
    const int nblk = ncg * ntile;
    int JC = c.wt_doubles / W;                      // rows per LDS chunk
    if (JC > N) JC = N;
    const double bias = c.prm.wbias;
    double* wt = WT();
    for (int b0 = 0; b0 < nblk; b0 += nwaves()) {
        const int b = b0 + wave_id();
        const bool have = b < nblk;
        const int cg = have ? b % ncg : 0, tile = have ? b / ncg : 0;
        const int k = cg * colw + lane() * C;
        const bool live = have && k < N;
        double acc[MT][C];
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int q = 0; q < C; ++q) acc[t][q] = 0.0;
        for (int jc = 0; jc < N; jc += JC) {
            const int jn = (N - jc) < JC ? (N - jc) : JC;
            block_sync();                           // the previous chunk has been consumed
            for (int p = tid(); p < jn * W; p += nthreads()) {
                int j = p / W, m = p - j * W;
                wt[p] = c.wsrc[(size_t)(jc + j) * c.mcap + m];
            }
            block_sync();
            if (live) {
                cgdp lrow = c.lsim + (size_t)jc * c.ld + k;
                const double* wrow = wt + tile * MT;
                int j = 0;
                for (; j + UNR <= jn; j += UNR) {
                    double a[UNR][C];
#pragma unroll
                    for (int u = 0; u < UNR; ++u) load_cols<C>(lrow + (size_t)(j + u) * c.ld, a[u]);
#pragma unroll
                    for (int u = 0; u < UNR; ++u)
#pragma unroll
                        for (int t = 0; t < MT; ++t) {
                            const double wv = wrow[(j + u) * W + t];
#pragma unroll
                            for (int q = 0; q < C; ++q) acc[t][q] = fma(wv, a[u][q], acc[t][q]);
                        }
                }
                for (; j < jn; ++j) {
                    double a1[C];
                    load_cols<C>(lrow + (size_t)j * c.ld, a1);
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        const double wv = wrow[j * W + t];
#pragma unroll
                        for (int q = 0; q < C; ++q) acc[t][q] = fma(wv, a1[q], acc[t][q]);
                    }
                }
            }
        }
        if (live) {
#pragma unroll
            for (int q = 0; q < C; ++q) {
                const int kk = k + q;
                if (kk < N) {
                    const double lw = c.lweight[kk], dn = c.den[kk];
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        const int m = tile * MT + t;
                        if (m < M)
                            c.w[(size_t)m * c.ldn + kk] =
                                (c.wsrc[(size_t)kk * c.mcap + m] + bias * lw * acc[t][q]) / dn;
                    }
                }
            }
        }
    }
    block_sync();
}

// Single-pass smoother for images whose whole operand panel fits in LDS (N x W doubles).
// lsim is read exactly ONCE per call: every lane keeps NT*8 VP accumulators for its C columns.
// Work split: wave w owns row slice w (all waves equally loaded for any N) and walks every
// column group; the row-slice partials go through an L2-resident scratch and are summed in a fixed
// order (deterministic).  When the column groups divide evenly among the waves (ncg % nwaves == 0,
// e.g. N = 1000 with C = 2) each wave instead owns whole column groups and writes results directly.
// Loads are software-pipelined two batches deep so the L2/HBM latency of batch b+1 hides under the
// FMAs of batch b.
template <int NT, int C>
VPK_DEVFN void smooth_full(EmCtx& c, int m0) {
    Shared& sh = SH();
    constexpr int W = NT * MT;
    // rows per prefetch batch: two batches are in flight per lane (16 rows x 16 B at C = 2 -- the bytes
    // in flight, not occupancy, are what hides the ~1.5 us loaded memory latency), fewer when the
    // accumulators already take most of the register file
    constexpr int UNR = (NT * C >= 8) ? 4 : 8;
    const int N = c.N;
    const int M = sh.M - m0 < W ? sh.M - m0 : W;    // VPs handled by this call: [m0, m0 + M)
    const double bias = c.prm.wbias;
    double* wt = WT();
    long long tq_ = clock_ticks();
    if (!(m0 == 0 && sh.ibuf[5] == W)) {            // not left in place by the E-step
        for (int p = tid(); p < N * W; p += nthreads()) {
            const int j = p / W, m = p - j * W;
            wt[p] = (m < M) ? c.wsrc[(size_t)j * c.mcap + m0 + m] : 0.0;
        }
        block_sync();
    }
    if (tid() == 0) sh.dbuf[8] += lap(tq_);
    const int colw = WAVE * C;
    const int ncg = (N + colw - 1) / colw;
    const int nw = nwaves();
    const bool direct = (ncg % nw) == 0;            // whole column groups per wave, no row slicing
    const int R = direct ? 1 : nw;                  // (the reduction below handles up to 8 row slices)
    const int slice = direct ? 0 : wave_id();
    const int jchunk = (N + R - 1) / R;
    const int j0 = slice * jchunk;
    const int j1 = (j0 + jchunk) < N ? (j0 + jchunk) : N;
    for (int cg = direct ? wave_id() : 0; cg < ncg; cg += direct ? nw : 1) {
        const int k = cg * colw + lane() * C;
        const bool live = k < N;
        double acc[W][C];
#pragma unroll
        for (int t = 0; t < W; ++t)
#pragma unroll
            for (int q = 0; q < C; ++q) acc[t][q] = 0.0;
        if (live) {
            cgdp lcol = c.lsim + k;
            double a0[UNR][C], a1[UNR][C];
            double wb[2][MT];                       // operand double buffer: one 8-VP group ahead
            int j = j0;
            const int nfull = (j1 - j0) / UNR;      // full batches
            if (nfull > 0) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) load_cols<C>(lcol + (size_t)(j + u) * c.ld, a0[u]);
#pragma unroll
                for (int t = 0; t < MT; ++t) wb[0][t] = wt[(size_t)j * W + t];
            }
            for (int b = 0; b < nfull; ++b) {
                const bool more = b + 1 < nfull;
                if (more) {
#pragma unroll
                    for (int u = 0; u < UNR; ++u) load_cols<C>(lcol + (size_t)(j + UNR + u) * c.ld, a1[u]);
                }
                // UNR * NT steps, each: prefetch the next step's 8 operands, then 8*C FMAs on the current
                // ones.  pin8 keeps the steps in order (registers stay bounded), the prefetch hides the
                // LDS latency under the FMAs.
#pragma unroll
                for (int st = 0; st < UNR * NT; ++st) {
                    const int u = st / NT, g = st % NT;
                    const int nu = (st + 1) / NT, ng = (st + 1) % NT;
                    int nrow = j + nu;                          // row of the next step
                    if (st + 1 == UNR * NT) nrow = more ? j + UNR : j;   // last step: next batch (or a harmless re-read)
                    const double* nw = wt + (size_t)nrow * W + ng * MT;
#pragma unroll
                    for (int t = 0; t < MT; ++t) wb[(st + 1) & 1][t] = nw[t];
#pragma unroll
                    for (int t = 0; t < MT; ++t)
#pragma unroll
                        for (int q = 0; q < C; ++q)
                            acc[g * MT + t][q] = fma(wb[st & 1][t], a0[u][q], acc[g * MT + t][q]);
#pragma unroll
                    for (int q = 0; q < C; ++q)
                        pin8(acc[g * MT][q], acc[g * MT + 1][q], acc[g * MT + 2][q], acc[g * MT + 3][q],
                             acc[g * MT + 4][q], acc[g * MT + 5][q], acc[g * MT + 6][q], acc[g * MT + 7][q]);
                }
                if (more) {
#pragma unroll
                    for (int u = 0; u < UNR; ++u)
#pragma unroll
                        for (int q = 0; q < C; ++q) a0[u][q] = a1[u][q];
                }
                j += UNR;
            }
            // the slice's last rows (fewer than a batch): all their loads are issued before the first is used -- one
            // memory round trip instead of one per row (N = 245: 7 such rows per slice and column group, a third of the
            // phase's time); same rows in the same order
            const int rem = j1 - j;
            if (rem > 0) {
#pragma unroll
                for (int u = 0; u < UNR - 1; ++u)
                    if (u < rem) load_cols<C>(lcol + (size_t)(j + u) * c.ld, a0[u]);
#pragma unroll
                for (int u = 0; u < UNR - 1; ++u) {
                    if (u >= rem) break;
                    const double* wr = wt + (size_t)(j + u) * W;
#pragma unroll
                    for (int t = 0; t < W; ++t) {
                        const double wv = wr[t];
#pragma unroll
                        for (int q = 0; q < C; ++q) acc[t][q] = fma(wv, a0[u][q], acc[t][q]);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < C; ++q) {
                const int kk = k + q;
                if (kk >= N) continue;
                if (direct) {
                    const double lw = c.lweight[kk], dn = c.den[kk];
#pragma unroll
                    for (int t = 0; t < W; ++t)
                        if (t < M)
                            c.w[(size_t)(m0 + t) * c.ldn + kk] =
                                (wt[(size_t)kk * W + t] + bias * lw * acc[t][q]) / dn;
                } else {
#pragma unroll
                    for (int t = 0; t < W; ++t)
                        if (t < M) c.part[((size_t)slice * c.mcap + t) * c.ldn + kk] = acc[t][q];
                }
            }
        }
    }
    if (!direct) {
        block_sync();
        if (tid() == 0) sh.dbuf[9] += lap(tq_);
        // Work items = (column, batch of RB VPs), columns fastest (coalesced), dealt round-robin to ALL threads: with one
        // thread per column only N of the 512 threads worked, each through M / RB dependent batches of L2 round trips.
        // All the partials of a batch are loaded before any is used (the stores to w keep the compiler from hoisting
        // loads); each (column, VP) is still summed over the slices in the fixed order 0..7.
        constexpr int RB = 4;
        const int nbatch = (M + RB - 1) / RB;
        for (int item = tid(); item < N * nbatch; item += nthreads()) {
            const int t0 = (item / N) * RB, kk = item - (item / N) * N;
            const double blw = bias * c.lweight[kk], dn = c.den[kk];
            cgdp pcol = c.part + kk;
            double v[RB][8];
#pragma unroll
            for (int u = 0; u < RB; ++u)
#pragma unroll
                for (int r = 0; r < 8; ++r)
                    v[u][r] = (t0 + u < M && r < R) ? pcol[((size_t)r * c.mcap + t0 + u) * c.ldn] : 0.0;
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                if (t0 + u >= M) break;
                double sum = 0.0;
#pragma unroll
                for (int r = 0; r < 8; ++r) sum += v[u][r];                                   // fixed order
                c.w[(size_t)(m0 + t0 + u) * c.ldn + kk] = (wt[(size_t)kk * W + t0 + u] + blw * sum) / dn;
            }
        }
    }
    block_sync();
    if (tid() == 0) sh.dbuf[10] += lap(tq_);
}

// lsim carries 8 rows more than the image has lines; the rows N .. 8 ceil(N / 8) - 1 are zero (smooth_rows walks them
// with zero operands where a slice is short or empty).  Once per image, after the matrix is in place.
VPK_DEVFN void zero_tail_rows(EmCtx& c) {
    const int N = c.N, jend = 8 * rs_jchunk(N);
    for (int p = tid(); p < (jend - N) * c.ld; p += nthreads()) c.lsim[(size_t)N * c.ld + p] = 0.0;
    block_sync();
}

// Row-sliced smoother: the same eight row slices and the same summation order as smooth_full, but no partial sum ever
// leaves the wave.  A wave owns 16 columns; its four rows of 16 lanes own the slices d and d + 4 (d = lane / 16), so the
// eight partials of a (column, VP) live in the four lanes {column, 16 + column, ...} of ONE wave and are summed through a
// 4.6 KB wave-private LDS scratch in the fixed order 0..7 -- no HBM/L2 round trip of the partials, no workgroup barrier
// before the results are written.  The w_ operands no longer come as wave-uniform broadcast reads (W / 2 ds_read_b128
// per row, as many LDS cycles as the FMAs take SIMD cycles): lane i of a row of 16 reads operand i (and 16 + i) of its
// slice's row ONCE and the FMAs take them through DPP row_newbcast (fmac8_row_bcast).  Per lane and row of a slice:
// one 8-byte lsim load (a row of 16 lanes = one 128-byte line), one or two 8-byte LDS reads, W FMAs.
template <int NT>
VPK_DEVFN void smooth_rows(EmCtx& c, int m0) {
    Shared& sh = SH();
    constexpr int W = NT * MT;
    constexpr int UNR = 4;                          // rows per load batch and slice; two batches are in flight
    const int N = uniform_int(c.N);
    m0 = uniform_int(m0);
    const int M = uniform_int(sh.M) - m0 < W ? uniform_int(sh.M) - m0 : W;    // VPs of this pass: [m0, m0 + M)
    const double bias = c.prm.wbias;
    double* wt = WT();
    long long tq_ = clock_ticks();
    const int jch = rs_jchunk(N), S = rs_sstride(jch, W);
    if (m0 != 0 || sh.ibuf[5] != RS_PANEL_FLAG + W) {   // not left in place by the E-step (passes; vpk_weight_matrix): stage it
        for (int p = tid(); p < N * W; p += nthreads()) {
            const int j = p / W, m = p - j * W;
            wt[rs_row(j, jch, S, W) + m] = (m < M) ? c.wsrc[(size_t)j * c.mcap + m0 + m] : 0.0;
        }
        for (int p = N * W + tid(); p < 8 * jch * W; p += nthreads()) {   // rows a short or empty slice does not have
            const int j = p / W;
            wt[rs_row(j, jch, S, W) + (p - j * W)] = 0.0;
        }
        block_sync();
    }
    if (tid() == 0) sh.dbuf[8] += lap(tq_);
    double* red = wt + rs_panel_doubles(jch, W) + wave_id() * RS_RED_DOUBLES;
    const int d = lane() >> 4, i = lane() & 15;
    const int jA0 = d * jch, jB0 = (d + 4) * jch;
    const double* oA = wt + (size_t)d * S + i;      // operand i of row r of the slice: oA[r * W] (and oA[r * W + 16])
    const double* oB = wt + (size_t)(d + 4) * S + i;
    const size_t ld = (size_t)uniform_int(c.ld), ldn = (size_t)uniform_int(c.ldn);
    cgdp lsim = c.lsim, lweight = c.lweight, den = c.den;   // (locals: the compiler barriers below would make it re-read c)
    gdp wout = c.w;
    // Every lane walks jch rows of both of its slices, also where a slice is short or empty (the last ones): the rows
    // N .. 8 jch - 1 exist in lsim as zeros (zero_tail_rows) and the operand rows of those "lines" are zero in the panel
    // (estep / the staging pass above), and fma(0, 0, acc) returns acc bit for bit (acc is never -0: it starts at +0
    // and a zero product is absorbed).  So the loop has no divergent branch, every load is unconditional with the
    // address (scalar row base) + (per-lane constant), and the compiler can count its waits.  The loads run one batch
    // of UNR rows ahead of the FMAs ACROSS column blocks: the last batch of a block requests the first rows of the
    // wave's next block, so only the first block of a call starts cold.
    const int nb = (jch + UNR - 1) / UNR;           // batches per column block; the last has jch - (nb - 1) UNR rows
    cgdp lbase = uniform_ptr(lsim);
    const unsigned rowbytes = (unsigned)ld * 8u;
    const int kstep = uniform_int(nwaves()) * 16;
    int k0 = uniform_int(wave_id()) * 16;
    if (k0 < N) {
        int k = k0 + i;
        int kc = k < N ? k : N - 1;                 // lanes past the last column stay active: they are operand sources
        unsigned offA = ((unsigned)jA0 * (unsigned)ld + (unsigned)kc) * 8u, offB = ((unsigned)jB0 * (unsigned)ld + (unsigned)kc) * 8u;
        double aA[UNR], aB[UNR], nA_[UNR], nB_[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int rn = u < jch ? u : jch - 1;
            cgdp rowp = (cgdp)((const VPK_GLOBAL char*)lbase + (size_t)rn * rowbytes);
            aA[u] = load_at(rowp, offA);
            aB[u] = load_at(rowp, offB);
        }
        for (;;) {
            const double lwk = lweight[kc];         // requested now, consumed after the row loop
            double dn = den[kc];
            const int k0n = k0 + kstep;
            const bool has_next = k0n < N;
            const int kn = k0n + i;
            const int kcn = has_next ? (kn < N ? kn : N - 1) : kc;
            const unsigned offAn = ((unsigned)jA0 * (unsigned)ld + (unsigned)kcn) * 8u, offBn = ((unsigned)jB0 * (unsigned)ld + (unsigned)kcn) * 8u;
            double accA[W], accB[W];
#pragma unroll
            for (int t = 0; t < W; ++t) { accA[t] = 0.0; accB[t] = 0.0; }
            double cA0 = oA[0], cA1 = W >= 24 ? oA[16] : 0.0, cB0 = oB[0], cB1 = W >= 24 ? oB[16] : 0.0;   // operands of row 0
            // one batch: request the rows of the following batch into (nxA, nxB), then the FMAs of this batch's rows
            // out of (cuA, cuB).  The two register sets swap roles from batch to batch (no copies: a copy would wait
            // for the loads it moves).
            auto batch = [&](int b, double (&cuA)[UNR], double (&cuB)[UNR], double (&nxA)[UNR], double (&nxB)[UNR])
                             __attribute__((always_inline)) {
                const int r = b * UNR;
                const bool lastb = b + 1 == nb;
                const int nrow = lastb ? jch - r : UNR;
                const int rnext = lastb ? 0 : r + UNR;          // first row of the batch requested now
                const unsigned oa = lastb ? offAn : offA, ob = lastb ? offBn : offB;
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    int rn = rnext + u;
                    rn = rn < jch ? rn : jch - 1;
                    cgdp rowp = (cgdp)((const VPK_GLOBAL char*)lbase + (size_t)rn * rowbytes);
                    nxA[u] = load_at(rowp, oa);
                    nxB[u] = load_at(rowp, ob);
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    if (u < nrow) {                 // wave-uniform
                        int rq = r + u + 1;         // the next row's operands are requested before this row's FMAs
                        rq = rq < jch ? rq : 0;     // (after the block's last row: row 0 again, for the next block)
                        const double* qA = oA + (size_t)rq * W;
                        const double* qB = oB + (size_t)rq * W;
                        const double xA0 = qA[0], xA1 = W >= 24 ? qA[16] : 0.0, xB0 = qB[0], xB1 = W >= 24 ? qB[16] : 0.0;
                        fmac8_row_bcast<0>(accA, cA0, cuA[u]);
                        if (W >= 16) fmac8_row_bcast<8>(accA + (W >= 16 ? 8 : 0), cA0, cuA[u]);
                        if (W >= 24) fmac8_row_bcast<0>(accA + (W >= 24 ? 16 : 0), cA1, cuA[u]);
                        if (W >= 32) fmac8_row_bcast<8>(accA + (W >= 32 ? 24 : 0), cA1, cuA[u]);
                        fmac8_row_bcast<0>(accB, cB0, cuB[u]);
                        if (W >= 16) fmac8_row_bcast<8>(accB + (W >= 16 ? 8 : 0), cB0, cuB[u]);
                        if (W >= 24) fmac8_row_bcast<0>(accB + (W >= 24 ? 16 : 0), cB1, cuB[u]);
                        if (W >= 32) fmac8_row_bcast<8>(accB + (W >= 32 ? 24 : 0), cB1, cuB[u]);
                        cA0 = xA0; cA1 = xA1; cB0 = xB0; cB1 = xB1;
                    }
                }
            };
            int b = 0;
            for (; b + 1 < nb; b += 2) {
                batch(b, aA, aB, nA_, nB_);
                batch(b + 1, nA_, nB_, aA, aB);
            }
            const bool odd = b < nb;
            if (odd) batch(b, aA, aB, nA_, nB_);    // the next block's first rows are in (nA_, nB_): moved after the rounds
        // the eight partials of every (VP, column) of this wave, summed in slice order: RS_TT VPs per round through the
        // wave's scratch [vp][column][slice]; lane (d, i) writes its slices d and d + 4 and finishes VP t0 + d of column i
        if (tid() == 0) sh.dbuf[9] += lap(tq_);     // row loops (wave 0)
        const double blw = bias * lwk;
        asm volatile("" : "+v"(dn));                // dn has arrived before the rounds: no wait inside them (a wait there
                                                    //   would also wait for the previous round's store)
        const double* wk = wt + rs_row(kc, jch, S, W);       // w_[kc][.]
        double* rw = red + (size_t)i * 9 + d;
        const double* rr_ = red + ((size_t)d * 16 + i) * 9;
#pragma unroll
        for (int t0 = 0; t0 < W; t0 += RS_TT) {
            if (t0 < M) {
#pragma unroll
                for (int u = 0; u < RS_TT; ++u) {
                    rw[(size_t)u * 16 * 9] = accA[t0 + u];
                    rw[(size_t)u * 16 * 9 + 4] = accB[t0 + u];
                }
                wave_lds_order();
                double sum = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) sum += rr_[q];                                      // fixed order
                const int t = t0 + d;
                if (t < M && k < N) wout[(size_t)(m0 + t) * ldn + k] = (wk[t] + blw * sum) / dn;
                wave_lds_order();
            }
        }
        if (tid() == 0) sh.dbuf[10] += lap(tq_);    // reduction rounds (wave 0)
            if (!has_next) break;
            if (odd) {
#pragma unroll
                for (int u = 0; u < UNR; ++u) { aA[u] = nA_[u]; aB[u] = nB_[u]; }
            }
            k0 = k0n; k = kn; kc = kcn; offA = offAn; offB = offBn;
        }
    }
    block_sync();
    if (tid() == 0) sh.dbuf[10] += lap(tq_);        // + waiting for the other waves
}

// ---------------------------------------------------------------------------------------------
// Sparse smoother (round 4, NOT the default: vpk_em_set_smoother(h, 2)): the same sums in the same order as smooth_rows /
// smooth_full, without the zero terms.  Built to test the lead "82-85 % of the operands are zeros" and measured SLOWER than
// the dense row-sliced kernel on the bench's batch (smoothing 114 ms of workgroup time per YUD batch against 84 ms; 58-62
// against 55 us per call at N = 364, M = 24): a wave issues at most one instruction every four cycles and the workgroup has
// two waves per SIMD, so what counts is instructions per wave, and the sparse kernel spends ~45 (mostly scalar: next set
// bit, slice boundary test, a test and a branch per VP, two v_readlane per weight) per staged row step where the dense
// kernel spends its W = 24 v_fmac_f64_dpp and almost nothing else -- six times fewer FMAs bought with more than six times
// the control instructions.  The LDS traffic (21 us estimated) and the staging (1 % of the time waiting for the DMA) are
// not what bounds it; the barrier per block costs 28 % (the waves own VPs, and VPs have unequal numbers of lines).  Kept
// as an option with its bit-equality test; DESIGN.md section 8.
//
// 82-85 % of the operands w_[line][vp] = p_vl * lweight are exact zeros: a line has a non-zero responsibility for two to
// four of ~20 hypotheses, exp underflows to 0 for the rest (sigma^2 <= 1e-6, :306).  fma(0, x, acc) returns acc bit for
// bit for a finite x (acc is never -0), so leaving those terms out changes nothing -- provided lsim holds no NaN / Inf
// (sh.ibuf[2], set from the row sums: a line of length 0).  The dense kernels cannot skip them: one of their FMA
// instructions covers four lines (slices) at once.  Here
//   * a WAVE owns up to four VPs (t = wave, wave + 8, ...), a LANE owns the columns k = lane, lane + 64, ... (CMAX per lane):
//     the accumulators of a (VP, column) never leave their lane;
//   * lsim is staged through LDS in blocks of SP_R consecutive rows by all threads (every element fetched once per call,
//     16-byte loads one block ahead of the block being used: the traffic of the dense kernels), two buffers, ONE
//     workgroup barrier per block;
//   * the wave's weights sit in registers, lane l holding w_[64 ci + l][t]; per block and VP a ballot gives the rows of
//     the block with a non-zero weight, and for each of them the wave reads the staged row (conflict-free 8-byte reads)
//     and issues ONE fma per column group with the weight as a scalar operand (v_readlane);
//   * the summation order of the dense kernels is kept: rows ascending, a partial per slice of jch = ceil(N / 8) rows,
//     the eight partials added in slice order (an empty slice adds +0) -- hence the same bits in every output
//     (tests/test_gpu_em.py compares the three smoothers with array_equal).
// Applies where smooth_rows applied and N <= 64 CMAX; everything else keeps its kernel.
// ---------------------------------------------------------------------------------------------
constexpr int SP_R = 16;                                // rows per staged block
static_assert((size_t)SP_R + 1 <= vpk::EM_LSIM_PAD_ROWS, "smooth_sparse stages rows up to 16 ceil(N / 16) - 1 plus one piece's overrun: em_layout must pad lsim for them");
constexpr int SP_CMAX = 7;                              // column groups of 64 per lane: N <= 448
VPK_DEV int sp_cgroups(int N) { return (N + WAVE - 1) / WAVE; }
VPK_DEV int sp_ldw(int C) { return ((C + 1) / 2) * 2 * WAVE; }   // staged row: whole 1 KB DMA pieces (128 doubles)
VPK_DEV int sp_ring(int C) { return C <= 6 ? 3 : 2; }           // staged blocks in LDS (one in use, the others in flight)
VPK_DEV bool sparse_smoother_fits(const EmCtx& c) {
    const int C = sp_cgroups(c.N);
    return WAVE == 64 && nwaves() == 8 && c.smoother == 2 && c.N > 0 && C <= SP_CMAX &&
           sp_ring(C) * SP_R * sp_ldw(C) <= c.wt_doubles;
}
template <int C>                                        // C = column groups of 64 in use: ceil(N / 64)
VPK_DEVFN void smooth_sparse(EmCtx& c, int m0) {
    Shared& sh = SH();
    constexpr int R = SP_R, NB = C <= 6 ? 3 : 2, VPW = 4;   // rows per block, ring size (sp_ring), VPs per wave
    constexpr int AHEAD = NB - 1;                   // blocks in flight ahead of the one in use
    constexpr int LDW = ((C + 1) / 2) * 2 * (WAVE >= 2 ? WAVE : 2);   // row stride of a staged row (doubles)
    constexpr int DPR = LDW / 128 > 0 ? LDW / 128 : 1;                 // DMA pieces per row
    constexpr int DPB = R * DPR / 8;                // DMA pieces per wave and block (8 waves: two rows' worth)
    constexpr int BPG = (WAVE >= R ? WAVE : R) / R; // blocks per group of 64 rows
    const int N = uniform_int(c.N);
    m0 = uniform_int(m0);
    const int M = uniform_int(sh.M) - m0 < 32 ? uniform_int(sh.M) - m0 : 32;   // VPs of this pass: [m0, m0 + M)
    const int jch = rs_jchunk(N);
    const int nblk = (N + R - 1) / R;
    const size_t ld = (size_t)uniform_int(c.ld), ldn = (size_t)uniform_int(c.ldn);
    const double bias = c.prm.wbias;
    cgdp lsim = uniform_ptr(c.lsim);
    cgdp lweight = c.lweight, den = c.den, pvl = c.pvl;
    gdp wout = c.w;
    double* buf = WT();                             // [NB][R][LDW]: the ring
    const unsigned buf_lds = lds_addr_of(buf);
    long long tq_ = clock_ticks();
    const int wv = uniform_int(wave_id()), ln = lane();
    // ---- this wave's weights: wreg[q][ci] = w_[64 ci + lane][m0 + wv + 8 q] = p_vl * lweight (weight_matrix :519).  All of
    //      them up front: the main loop then has no vector-memory operation but its DMA, whose completion it counts ----
    double wreg[VPW][C];
    {
        // unconditional loads (indices clamped into the arrays) so that they are issued together, selected afterwards
        double lwv[C], raw[VPW][C];
#pragma unroll
        for (int ci = 0; ci < C; ++ci) {
            const int j = ci * WAVE + ln;
            lwv[ci] = lweight[j < N ? j : N - 1];
        }
#pragma unroll
        for (int q = 0; q < VPW; ++q) {
            const int t = wv + 8 * q;
            cgdp row = pvl + (size_t)(m0 + (t < M ? t : M - 1)) * ldn;
#pragma unroll
            for (int ci = 0; ci < C; ++ci) {
                const int j = ci * WAVE + ln;
                raw[q][ci] = row[j < N ? j : N - 1];
            }
        }
#pragma unroll
        for (int q = 0; q < VPW; ++q)
#pragma unroll
            for (int ci = 0; ci < C; ++ci) {
                const double prod = raw[q][ci] * lwv[ci];
                wreg[q][ci] = (ci * WAVE + ln < N && wv + 8 * q < M) ? prod : 0.0;
            }
    }
    double part[VPW][C], tot[VPW][C];
#pragma unroll
    for (int q = 0; q < VPW; ++q)
#pragma unroll
        for (int cc = 0; cc < C; ++cc) { part[q][cc] = 0.0; tot[q][cc] = 0.0; }
    int bound[VPW];                                 // first row of the slice after the one part[q] belongs to
#pragma unroll
    for (int q = 0; q < VPW; ++q) bound[q] = jch;
    double blwk[C], dnk[C];                         // the results' per-column constants (:522), fetched now for the same reason
#pragma unroll
    for (int cc = 0; cc < C; ++cc) {
        const int k = cc * WAVE + ln;
        const int kc = k < N ? k : N - 1;
        blwk[cc] = bias * lweight[kc];
        dnk[cc] = den[kc];
        pin1(blwk[cc]); pin1(dnk[cc]);
    }
    // every weight has arrived before the first DMA is issued: from here on the compiler has no vector-memory operation of
    // its own in flight and puts no s_waitcnt vmcnt into the main loop (one there would wait for the whole ring)
#pragma unroll
    for (int q = 0; q < VPW; ++q)
#pragma unroll
        for (int ci = 0; ci < C; ++ci) pin1(wreg[q][ci]);
    wait_vm<0>();
    // ---- staging by LDS-DMA: piece p of a block = (row p / DPR, 128 doubles p % DPR); wave w issues the pieces w, w + 8, ..
    //      Rows up to 8 ceil(N / 8) - 1 are zeros (zero_tail_rows), rows up to N + EM_LSIM_PAD_ROWS - 1 belong to lsim
    //      (em_layout): a block's last rows and a piece that runs past its row's ld doubles into the next row stay inside
    //      the matrix; what they hold meets zero operand bits / columns no lane owns a result for ----
    auto issue = [&](int blk) __attribute__((always_inline)) {
        const unsigned dst = buf_lds + (unsigned)((blk % NB) * R * LDW * 8);
#pragma unroll
        for (int u = 0; u < DPB; ++u) {
            const int p = wv + 8 * u;
            const int r = p / DPR, x = p - r * DPR;
            cgdp src = lsim + ((size_t)(blk * R + r) * ld + (size_t)x * 128);
            lds_dma16((unsigned)ln * 16u, (const void*)uniform_ptr(src), (unsigned)uniform_int((int)(dst + (unsigned)((r * LDW + x * 128) * 8))));
        }
    };
    issue(0);
    if (AHEAD > 1 && nblk > 1) issue(1);
    if (AHEAD > 2 && nblk > 2) issue(2);
    if (tid() == 0) sh.dbuf[8] += lap(tq_);
    // ---- the blocks: group ci of 64 rows = BPG blocks; (ci, q) static so that the accumulators stay in registers ----
#pragma unroll
    for (int ci = 0; ci < C; ++ci) {
        if (ci * BPG >= nblk) break;                // uniform
        unsigned long long nz[VPW];
#pragma unroll
        for (int q = 0; q < VPW; ++q) nz[q] = wave_ballot(wreg[q][ci] != 0.0);
        for (int b8 = 0; b8 < BPG; ++b8) {
            const int blk = ci * BPG + b8;
            if (blk >= nblk) break;                 // uniform
            // this wave's pieces of block blk have landed (the pieces of the AHEAD - 1 later blocks may still be in flight) ...
            const int later = nblk - 1 - blk;
            if (AHEAD >= 2 && later >= AHEAD - 1) wait_vm<(AHEAD - 1) * DPB>(); else wait_vm<0>();
            raw_barrier();                          // ... and every wave's; everybody is done with block blk - 1
            if (blk + AHEAD < nblk) issue(blk + AHEAD);   // into the buffer block blk - 1 used
            const double* rows = buf + (size_t)(blk % NB) * R * LDW + ln;
            unsigned mq[VPW], any = 0;              // per VP: the rows of this block with a non-zero weight; their union
#pragma unroll
            for (int q = 0; q < VPW; ++q) { mq[q] = (unsigned)(nz[q] >> (b8 * R)) & ((1u << R) - 1u); any |= mq[q]; }
            if (any == 0) continue;                 // uniform
            // One staged row serves all of the wave's VPs that have a weight for it; the row of the NEXT step is requested
            // before the FMAs of the current one (two register sets that swap roles).
            auto read_row = [&](int bit, double (&v)[C]) __attribute__((always_inline)) {
                const double* rp = rows + (size_t)bit * LDW;
#pragma unroll
                for (int cc = 0; cc < C; ++cc) v[cc] = rp[cc * WAVE];
            };
            int bit = __builtin_ctz(any);
            any &= any - 1;
            double va[C], vb[C];
            read_row(bit, va);
            auto step = [&](double (&cur)[C], double (&nxt)[C]) __attribute__((always_inline)) {
                const int cb = bit;
                const bool more = any != 0;
                bit = more ? __builtin_ctz(any) : cb;   // (after the last row: the same row once more -- the reads are issued
                any &= any - 1;                         //  unconditionally so that the compiler can count them: a conditional
                read_row(bit, nxt);                     //  request makes it wait for ALL outstanding reads before the FMAs)
                const int j = ci * WAVE + b8 * R + cb;
#pragma unroll
                for (int q = 0; q < VPW; ++q) {
                    if (!((mq[q] >> cb) & 1u)) continue;    // uniform
                    while (j >= bound[q]) {         // the row opens a later slice: close the current partial
#pragma unroll
                        for (int cc = 0; cc < C; ++cc) { tot[q][cc] += part[q][cc]; part[q][cc] = 0.0; }
                        bound[q] += jch;
                    }
                    const double wj = readlane_f64(wreg[q][ci], b8 * R + cb);
#pragma unroll
                    for (int cc = 0; cc < C; ++cc) part[q][cc] = fma(wj, cur[cc], part[q][cc]);
                }
                return more;
            };
            for (;;) {
                if (!step(va, vb)) break;
                if (!step(vb, va)) break;
            }
        }
    }
    if (tid() == 0) sh.dbuf[9] += lap(tq_);
    // ---- results: w[m][k] = (w_[k][m] + bias lweight[k] sum) / den[k]  (:522) ----
#pragma unroll
    for (int cc = 0; cc < C; ++cc) {
        const int k = cc * WAVE + ln;
        if (k < N) {
#pragma unroll
            for (int q = 0; q < VPW; ++q) {
                const int t = wv + 8 * q;
                if (t < M) wout[(size_t)(m0 + t) * ldn + k] = (wreg[q][cc] + blwk[cc] * (tot[q][cc] + part[q][cc])) / dnk[cc];
            }
        }
    }
    block_sync();                                   // (also: nobody reads the ring any more -- the panel region is free)
    if (tid() == 0) sh.dbuf[10] += lap(tq_);
}
VPK_DEVFN void smooth_sparse_any(EmCtx& c, int m0) {
    switch (sp_cgroups(c.N)) {
        case 1: smooth_sparse<1>(c, m0); break;
        case 2: smooth_sparse<2>(c, m0); break;
        case 3: smooth_sparse<3>(c, m0); break;
        case 4: smooth_sparse<4>(c, m0); break;
        case 5: smooth_sparse<5>(c, m0); break;
        case 6: smooth_sparse<6>(c, m0); break;
        default: smooth_sparse<7>(c, m0); break;
    }
}

// (smooth and smooth_dispatch are inlined into their callers: as functions of their own they cost two more levels of callee-saved
//  register saves and restores -- scratch memory, i.e. HBM round trips at the stress shape -- per E-step for a chain of ifs)
VPK_DEV void smooth_dispatch(EmCtx& c);
VPK_DEV void smooth(EmCtx& c) {
    smooth_dispatch(c);
    if (tid() == 0) SH().ibuf[5] = 0;               // the E-step's panel is valid for one smoothing only
    block_sync();
}
VPK_DEV void smooth_dispatch(EmCtx& c) {
    Shared& sh = SH();
    const int M = sh.M, N = c.N;
    if (!c.prm.use_weights) {   // lsim == 0 and lweight == 1 (:180,:235): w = p_vl
        for (int m = 0; m < M; ++m)
            for (int k = tid(); k < N; k += nthreads()) c.w[(size_t)m * c.ldn + k] = c.wsrc[(size_t)k * c.mcap + m];
        block_sync();
        return;
    }
    if (M == 0) return;
    const int plan = smooth_plan(c, M);
    if (WAVE == 64 && (sh.ibuf[5] >= RS_PANEL_FLAG || plan == 2 || plan == 3)) {   // (an E-step's panel decides; none: the plan)
        if (sparse_smoother_fits(c) && sh.ibuf[2] == 0) {   // the zero terms left out (same sums, same order, same bits)
            for (int m0 = 0; m0 < M; m0 += 32) smooth_sparse_any(c, m0);
            return;
        }
        const int wpass = plan == 3 ? rs_wfit(c) : 32;      // VPs per pass
        for (int m0 = 0; m0 < M; m0 += wpass) {
            const int mm = (M - m0) < wpass ? (M - m0) : wpass;
            if (mm <= 8) smooth_rows<1>(c, m0);
            else if (mm <= 16) smooth_rows<2>(c, m0);
            else if (mm <= 24) smooth_rows<3>(c, m0);
            else smooth_rows<4>(c, m0);
        }
        return;
    }
    // single-pass kernel on as many VPs as the LDS panel holds (N x wfit doubles, wfit a multiple of the VP
    // tile, at most 32 accumulator sets per lane); more VPs than that take further passes over lsim
    int wfit = (int)((c.wt_doubles / N) / MT) * MT;
    if (wfit > 32) wfit = 32;
    if (wfit >= MT) {
        for (int m0 = 0; m0 < M; m0 += wfit) {
            const int mm = (M - m0) < wfit ? (M - m0) : wfit;
            if (N > WAVE) {
                if (mm <= 8) smooth_full<1, 2>(c, m0);
                else if (mm <= 16) smooth_full<2, 2>(c, m0);
                else if (mm <= 24) smooth_full<3, 2>(c, m0);
                else smooth_full<4, 2>(c, m0);
            } else {
                if (mm <= 8) smooth_full<1, 1>(c, m0);
                else if (mm <= 16) smooth_full<2, 1>(c, m0);
                else if (mm <= 24) smooth_full<3, 1>(c, m0);
                else smooth_full<4, 1>(c, m0);
            }
        }
        return;
    }
    if (N > WAVE) smooth_blocks<2, 8>(c);
    else smooth_blocks<1, 4>(c);
}

}  // namespace vpk
#endif
