// em_vpset.hpp -- VP set maintenance inside the EM: merge_vps, the two-cluster agglomeration (global-memory and LDS-resident) and
// split_best_vp.
// One part of em_device.hpp (the conventions, and why the unit is compiled with -ffp-contract=off, are there).
#ifndef VPK_EM_VPSET_HPP_
#define VPK_EM_VPSET_HPP_

#include "em_ctx.hpp"
#include "em_linalg.hpp"
#include "em_estep.hpp"
#include "em_smooth.hpp"
#include "em_assign.hpp"
#include "em_mstep.hpp"

namespace vpk {

// ---------------------------------------------------------------------------------------------
// merge_vps (vp_localisation.py:633-697)
// ---------------------------------------------------------------------------------------------
template <int MEASURE = VPK_DIST_ANGLE>
VPK_DEVFN void merge_vps(EmCtx& c, bool use_next, double thresh, double max_stdd) {
    Shared& sh = SH();
    const int N = c.N;
    for (int guard = 0; guard < 4 * MAXM; ++guard) {
        const int M = sh.M;
        if (M <= 1) break;
        double* X = use_next ? sh.nxt : sh.cur;
        double bv = 1e300;
        int bi = 0x7fffffff;
        for (int p = tid(); p < M * M; p += nthreads()) {
            int j = p / M, k = p % M;
            double d = X[3 * j] * X[3 * k] + X[3 * j + 1] * X[3 * k + 1] + X[3 * j + 2] * X[3 * k + 2];
            double ang = (j == k) ? PI_D : fabs(acos(clip(fabs(clip(d, -1.0, 1.0)), -1.0, 1.0)));  // :691-696
            if (ang < bv || (ang == bv && p < bi)) { bv = ang; bi = p; }
        }
        block_argmin(sh, bv, bi);                             // first row-major minimum (:650)
        if (!(bv < thresh)) break;                            // :655,:679-680
        const int j = bi / M, k = bi % M;
        estep<MEASURE>(c, X);                                 // :658 (at the caller's index, under the caller's measure)
        smooth(c);
        if (wave_id() == 0) {                                 // newVP from w[j] + w[k] (:661)
            cgdp wj = c.w + (size_t)j * c.ldn;
            cgdp wk = c.w + (size_t)k * c.ldn;
            double wmax = -1e300;
            for (int n = lane(); n < N; n += WAVE) wmax = nanmax(wmax, wj[n] + wk[n]);
            wmax = wave_max(wmax);
            bool valid = N > 0 && (wmax > 0 || wmax < 0);
            double sv = 0, sp = 0;
            cgdp lj = c.lvsq + (size_t)j * c.ldn;
            cgdp lk = c.lvsq + (size_t)k * c.ldn;
            cgdp pj = c.pvl + (size_t)j * c.ldn;
            cgdp pk = c.pvl + (size_t)k * c.ldn;
            for (int n = lane(); n < N; n += WAVE) {
                double pq = pk[n] + pj[n];
                sv += 0.5 * (lj[n] + lk[n]) * pq;             // :664
                sp += pq;                                     // :663
            }
            sv = wave_sum(sv);
            sp = wave_sum(sp);
            double vp[3] = {0, 0, 0};
            if (valid) wave_null_vector(c.l, N, [=](int n) { return (wj[n] + wk[n]) / wmax; }, vp);
            if (lane() == 0) {
                double sk = exp(log(sv) - log(sp));
                sh.s[k] = sk;                                 // :666 written BEFORE the abort test
                int ok = valid && !(sk > max_stdd);           // :668 (the EM passes the default, 0.01)
                if (ok) {
                    double sg = sign_np(vp[2]);
                    X[3 * k] = vp[0] * sg; X[3 * k + 1] = vp[1] * sg; X[3 * k + 2] = vp[2] * sg;   // :672
                    for (int m = 0; m < M; ++m) sh.removed[m] = (m == j);                            // :674-675
                }
                sh.ibuf[0] = ok;
            }
        }
        block_sync();
        if (!sh.ibuf[0]) break;
        compact_vps(c);
    }
    block_sync();
}

// ---------------------------------------------------------------------------------------------
// 2-cluster average-linkage agglomeration == sklearn AgglomerativeClustering(linkage='average',
// connectivity=D, n_clusters=2, metric='precomputed') as called at vp_localisation.py:574-578.
// sklearn 0.18..1.7 behaviour restated: edges are the non-zero entries of D + D^T; repeatedly
// merge the closest connected pair; a neighbour shared by both gets (n_a d_a + n_b d_b)/(n_a+n_b),
// a neighbour of only one keeps its distance; the full tree is built and cut at the root, the
// cluster formed LAST (node 2n-3) gets label 0 (_hc_cut pops the larger node id first).
// Exact ties between candidate merges are resolved by Python heap order in sklearn; here by the
// smallest matrix position, and VPK_EM_FLAG_SPLIT_TIE is raised.
// D: n x n working copy in global memory (destroyed); member: n ints; labels -> member (0/1).
// ---------------------------------------------------------------------------------------------
VPK_DEVFN void cluster2(Shared&, int n, gdp D, gip member, gip csize) {
    Shared& sh = SH();
    for (int p = tid(); p < n * n; p += nthreads()) {
        int a = p / n, b = p % n;
        double v = D[p];
        if (a == b || !(v + D[(size_t)b * n + a] != 0.0)) D[p] = -1.0;   // no edge
    }
    for (int a = tid(); a < n; a += nthreads()) { member[a] = a; csize[a] = 1; }
    block_sync();
    int last_slot = -1;
    for (int t = 0; t < n - 2; ++t) {
        double bv = 1e300;
        int bi = 0x7fffffff;
        int ties = 0;
        for (int p = tid(); p < n * n; p += nthreads()) {
            int a = p / n, b = p % n;
            if (a <= b || csize[a] == 0 || csize[b] == 0) continue;
            double v = D[p];
            if (v < 0) continue;
            if (v < bv) { bv = v; bi = p; ties = 0; }
            else if (v == bv) { ties = 1; }
        }
        const double myv = bv;
        block_argmin(sh, bv, bi);
        if (bi == 0x7fffffff) {                               // graph exhausted: disconnected
            if (tid() == 0) sh.flags |= VPK_EM_FLAG_SPLIT_DISCONNECTED;
            break;
        }
        // tie detection: the winning value occurs at more than one candidate position
        if (tid() == 0) sh.ibuf[1] = 0;
        block_sync();
        if (myv == bv) atomic_add_int(&sh.ibuf[1], 1 + ties);
        block_sync();
        const int a = bi / n, b = bi % n;                     // a > b; the merged cluster lives in slot a
        const int na = csize[a], nb = csize[b];
        block_sync();
        for (int cidx = tid(); cidx < n; cidx += nthreads()) {
            if (cidx == a || cidx == b || csize[cidx] == 0) continue;
            double da = D[(size_t)a * n + cidx], db = D[(size_t)b * n + cidx];
            double nv;
            if (da >= 0 && db >= 0)
                nv = (na * da + nb * db) / (double)(na + nb);  // average_merge
            else
                nv = da >= 0 ? da : db;                        // only one side connected (or none: -1)
            D[(size_t)a * n + cidx] = nv;
            D[(size_t)cidx * n + a] = nv;
        }
        for (int q = tid(); q < n; q += nthreads())
            if (member[q] == b) member[q] = a;
        block_sync();
        if (tid() == 0) {
            csize[a] = na + nb;
            csize[b] = 0;
            if (sh.ibuf[1] >= 2) sh.flags |= VPK_EM_FLAG_SPLIT_TIE;
        }
        last_slot = a;
        block_sync();
    }
    for (int q = tid(); q < n; q += nthreads()) member[q] = (member[q] == last_slot) ? 0 : 1;
    block_sync();
}

// Same algorithm for small sets (the usual case: the lines of one VP; <= 72 lines in the YUD-shape bench) out of LDS.  D is an
// n x ld matrix in LDS (ld odd, -1 = no edge; a merged-away slot's row and column are set to -1, so the search needs no
// activity test per entry).  Per merge the active rows a are walked with lanes over the columns b < a (consecutive LDS
// words, no index decoding), every lane keeps its own best (distance, position), and ONE cross-lane arg-min per wave ends
// the search -- a cross-lane reduction of a double + index costs ~1000 cycles on this part (scripts/ubench/wave_reduce.hip),
// as much as walking 30 rows, so the design minimises reductions, not LDS reads.  (Round 1 decoded a triangular pair index
// per entry: ~10 us per merge; a per-row nearest-neighbour cache with a reduction per rescanned row was no faster.)
// The matrix is the head of the LDS panel (WT()); behind it: member / csize [n] ints each.
// Two bodies, same comparisons, same labels and flags: cluster2_lds_wave (rounds 2-6) has ONE wave do everything, so a merge
// costs no workgroup barrier but the other waves wait for n - 2 walks of the whole triangle; cluster2_lds_block deals the
// walk's trips of four rows to all waves and pays two barriers per merge.
constexpr int CLUSTER_LDS_MAX = 128;
VPK_DEV long long cluster_lds_doubles(int n) { return (long long)n * (n | 1) + (long long)n + 4; }
VPK_DEV int* cluster_lds_labels(double* D, int n) {
    return reinterpret_cast<int*>(D + (size_t)n * (n | 1));
}
VPK_DEVFN void cluster2_lds_wave(int n) {
    Shared& sh = SH();
    // the matrix sits at the start of the LDS panel; deriving the pointer from the LDS symbol HERE (not taking it as
    // an argument of this non-inlined function) is what makes the accesses ds_read / ds_write instead of flat_*
    double* D = WT();
    const int ld = n | 1;
    int* member = cluster_lds_labels(D, n);
    int* csize = member + n;
    for (int a = tid(); a < n; a += nthreads()) { member[a] = a; csize[a] = 1; }
    block_sync();
    if (wave_id() == 0) {
        unsigned long long act[2];
        act[0] = n >= 64 ? ~0ull : ((1ull << n) - 1);
        act[1] = n > 64 ? (n >= 128 ? ~0ull : ((1ull << (n - 64)) - 1)) : 0ull;
        int last_slot = -1;
        bool tie_seen = false, disconnected = false;
        for (int t = 0; t < n - 2; ++t) {
            // Branch-free search, four rows per trip (their LDS reads are in flight together).  Distances are >= 0, so
            // their bit patterns order like unsigned integers, and "no edge" (-1.0: sign bit set) is larger than every
            // distance: one 64-bit integer compare per entry, no validity test.
            typedef unsigned long long u64;
            const u64 NONE = 0x7fe0000000000000ull;              // above every finite distance, below -1.0's pattern
            u64 bk = NONE;
            int bi = 0x7fffffff;
            int ties = 0;
            for (int c0 = 0; c0 < n; c0 += WAVE) {
                const int bq = c0 + lane();
                for (int a0 = (c0 > 0 ? c0 : 1); a0 < n; a0 += 4) {
                    u64 k[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int a = a0 + u;
                        const bool in = a < n && bq < a;
                        k[u] = in ? __double_as_longlong(D[(in ? a : 0) * ld + (in ? bq : 0)]) : ~0ull;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int pos = (a0 + u) * ld + bq;
                        const bool eq = k[u] == bk && k[u] < NONE;
                        const bool lt = k[u] < bk;
                        ties = lt ? 0 : (eq ? 1 : ties);
                        bi = (lt || (eq && pos < bi)) ? pos : bi;     // equal distances: the smallest position
                        bk = lt ? k[u] : bk;
                    }
                }
            }
            double bv = bk < NONE ? __longlong_as_double((long long)bk) : 1e300;
            if (!(bk < NONE)) bi = 0x7fffffff;
            const double myv = bv;
            wave_argmin(bv, bi);
            if (bi == 0x7fffffff) { disconnected = true; break; }
            if (wave_sum_int(myv == bv ? 1 + ties : 0) >= 2) tie_seen = true;
            const int ma = bi / ld, mb = bi - ma * ld;         // ma > mb; the merged cluster lives in slot ma
            const int na = csize[ma], nb = csize[mb];
            for (int cidx = lane(); cidx < n; cidx += WAVE) {
                if (cidx == ma || cidx == mb) continue;
                const double da = D[ma * ld + cidx], db = D[mb * ld + cidx];
                double nv;
                if (da >= 0 && db >= 0)
                    nv = (na * da + nb * db) / (double)(na + nb);  // average_merge
                else
                    nv = da >= 0 ? da : db;                        // only one side connected (or none: -1)
                D[ma * ld + cidx] = nv;                            // (dead slots hold -1 in every row: they stay -1)
                D[cidx * ld + ma] = nv;
                D[mb * ld + cidx] = -1.0;                          // slot mb leaves the search
                D[cidx * ld + mb] = -1.0;
            }
            if (lane() == 0) { D[ma * ld + mb] = -1.0; D[mb * ld + ma] = -1.0; }
            for (int q = lane(); q < n; q += WAVE)
                if (member[q] == mb) member[q] = ma;
            wave_sync();
            if (lane() == 0) { csize[ma] = na + nb; csize[mb] = 0; }
            wave_sync();
            act[mb >> 6] &= ~(1ull << (mb & 63));
            last_slot = ma;
        }
        for (int q = lane(); q < n; q += WAVE) member[q] = (member[q] == last_slot) ? 0 : 1;
        if (lane() == 0) {
            if (tie_seen) sh.flags |= VPK_EM_FLAG_SPLIT_TIE;
            if (disconnected) sh.flags |= VPK_EM_FLAG_SPLIT_DISCONNECTED;
        }
    }
    block_sync();
}

// The whole workgroup on every merge.  The search's trips (four rows of one 64-column block, in the one-wave body's order)
// are dealt to the waves round robin; a wave walks its trips as above and ends with its own arg-min.  The waves' results
// -- minimum, its smallest position, and how often the minimum occurred (1 + the lane's tie mark, over the lanes that hold
// it) -- go through sh.red_v / sh.red_i behind ONE barrier, and every wave reduces the (at most 16) candidates itself:
// smallest distance, smallest position among equal distances, and the tie count summed over the waves whose minimum is
// the global one (>= 2 exactly when the one-wave count is: the minimum sits at more than one position).  Every decision
// that leaves the loop is taken from these exchanged words, so all waves take it together.  The update (Lance-Williams
// average, the -1 row and column of the dead slot, member) has one slot per thread; a second barrier closes the merge.
// csize of the merged pair is written by thread 0 AFTER that barrier and read after the next merge's first one: the
// search in between does not look at it.
// With one wave (the host build: one thread) this is the one-wave walk.
VPK_DEVFN void cluster2_lds_block(int n) {
    Shared& sh = SH();
    double* D = WT();                                         // (from the LDS symbol, as above)
    const int ld = n | 1;
    int* member = cluster_lds_labels(D, n);
    int* csize = member + n;
    for (int a = tid(); a < n; a += nthreads()) { member[a] = a; csize[a] = 1; }
    block_sync();
    typedef unsigned long long u64;
    const u64 NONE = 0x7fe0000000000000ull;                   // above every finite distance, below -1.0's pattern
    constexpr int NOPOS = 0x7fffffff;
    const int nw = nwaves() < 16 ? nwaves() : 16;             // red_i holds [position | tie count] x 16
    const int w = wave_id();
    int last_slot = -1;
    bool tie_seen = false, disconnected = false;
    for (int t = 0; t < n - 2; ++t) {
        u64 bk = NONE;
        int bi = NOPOS;
        int ties = 0;
        int trip0 = 0;                                        // trips of the column blocks before this one
        for (int c0 = 0; c0 < n; c0 += WAVE) {
            const int bq = c0 + lane();
            const int astart = c0 > 0 ? c0 : 1;
            const int ntrips = (n - astart + 3) / 4;
            int first = (w - trip0) % nw;                     // this wave's first trip in the block
            if (first < 0) first += nw;
            for (int k = (w < nw ? first : ntrips); k < ntrips; k += nw) {
                const int a0 = astart + 4 * k;
                u64 key[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int a = a0 + u;
                    const bool in = a < n && bq < a;
                    key[u] = in ? __double_as_longlong(D[(in ? a : 0) * ld + (in ? bq : 0)]) : ~0ull;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int pos = (a0 + u) * ld + bq;
                    const bool eq = key[u] == bk && key[u] < NONE;
                    const bool lt = key[u] < bk;
                    ties = lt ? 0 : (eq ? 1 : ties);
                    bi = (lt || (eq && pos < bi)) ? pos : bi;     // equal distances: the smallest position
                    bk = lt ? key[u] : bk;
                }
            }
            trip0 += ntrips;
        }
        double bv = bk < NONE ? __longlong_as_double((long long)bk) : 1e300;
        if (!(bk < NONE)) bi = NOPOS;
        const double myv = bv;
        wave_argmin(bv, bi);
        const int cnt = wave_sum_int((myv == bv && bi != NOPOS) ? 1 + ties : 0);
        if (lane() == 0 && w < nw) { sh.red_v[w] = bv; sh.red_i[w] = bi; sh.red_i[16 + w] = cnt; }
        block_sync();
        double gv = sh.red_v[0];
        int gi = sh.red_i[0];
        for (int k = 1; k < nw; ++k) {
            const double u = sh.red_v[k];
            const int j = sh.red_i[k];
            const bool take = (u < gv) || (u == gv && j < gi);
            gv = take ? u : gv;
            gi = take ? j : gi;
        }
        gi = uniform_int(gi);
        if (gi == NOPOS) { disconnected = true; break; }      // graph exhausted (every wave reads the same words)
        int gcnt = 0;
        for (int k = 0; k < nw; ++k) gcnt += (sh.red_v[k] == gv && sh.red_i[k] != NOPOS) ? sh.red_i[16 + k] : 0;
        if (gcnt >= 2) tie_seen = true;
        const int ma = gi / ld, mb = gi - ma * ld;            // ma > mb; the merged cluster lives in slot ma
        const int na = csize[ma], nb = csize[mb];
        for (int cidx = tid(); cidx < n; cidx += nthreads()) {
            if (member[cidx] == mb) member[cidx] = ma;
            if (cidx == ma || cidx == mb) continue;
            const double da = D[ma * ld + cidx], db = D[mb * ld + cidx];
            double nv;
            if (da >= 0 && db >= 0)
                nv = (na * da + nb * db) / (double)(na + nb);  // average_merge
            else
                nv = da >= 0 ? da : db;                        // only one side connected (or none: -1)
            D[ma * ld + cidx] = nv;                            // (dead slots hold -1 in every row: they stay -1)
            D[cidx * ld + ma] = nv;
            D[mb * ld + cidx] = -1.0;                          // slot mb leaves the search
            D[cidx * ld + mb] = -1.0;
        }
        if (tid() == 0) { D[ma * ld + mb] = -1.0; D[mb * ld + ma] = -1.0; }
        block_sync();
        if (tid() == 0) { csize[ma] = na + nb; csize[mb] = 0; }
        last_slot = ma;
    }
    for (int q = tid(); q < n; q += nthreads()) member[q] = (member[q] == last_slot) ? 0 : 1;
    if (tid() == 0) {
        if (tie_seen) sh.flags |= VPK_EM_FLAG_SPLIT_TIE;
        if (disconnected) sh.flags |= VPK_EM_FLAG_SPLIT_DISCONNECTED;
    }
    block_sync();
}

// mode: EmCtx::smoother -- 1 selects the earlier form, as it does in the other phases (same bits either way).  Below 32 lines
// the two barriers per merge cost more than the shared walk saves (measured per launch of vpk_cluster2, one wave | workgroup:
// n = 9: 16 | 24 us, 24: 61 | 68, 28: 78 | 80, 32: 96 | 91, 48: 189 | 141, 64: 312 | 201, 72: 443 | 243, 126: 1606 | 583).
constexpr int CLUSTER_BLOCK_MIN = 32;
VPK_DEV void cluster2_lds(int n, int mode) {
    if (mode == 1 || n < CLUSTER_BLOCK_MIN) cluster2_lds_wave(n); else cluster2_lds_block(n);
}

// ---------------------------------------------------------------------------------------------
// split_best_vp (vp_localisation.py:527-630).  Expects w = weight matrix of sh.cur.
// Returns, to every thread alike, what it changed of the state an E-step + smoother of sh.cur left behind: SPLIT_WROTE_VPS --
// sh.cur / sh.s / sh.M (a split happened) --, SPLIT_WROTE_PVL -- the slot's p_vl rows (the directions of a very large set
// were staged there).  0: w, lvsq and p_vl still belong to sh.cur, and the caller need not evaluate them again.  (The LDS
// panel, assoc, idx and cl are overwritten in every case; nothing reads them before their next writer.)
// ---------------------------------------------------------------------------------------------
constexpr int SPLIT_WROTE_VPS = 1, SPLIT_WROTE_PVL = 2;
VPK_DEVFN int split_vp(EmCtx& c) {
    Shared& sh = SH();
    const int M = sh.M, N = c.N;
    if (M == 0 || c.cl == nullptr) return 0;
    long long tq_ = clock_ticks();
    assign_lines(c, false);                                   // weightIndices (:536) == vpAssoc (:551)
    double wmx = -1e300;
    for (int m = 0; m < M; ++m)
        for (int n = tid(); n < N; n += nthreads()) wmx = nanmax(wmx, c.w[(size_t)m * c.ldn + n]);
    wmx = block_max(sh, wmx);                                 // weightMatrix.max() (:539)
    // per VP: std of the folded line angle over lines with greedy weight > 0 (:541-544)
    for (int m = wave_id(); m < M; m += nwaves()) {
        int cnt = 0, call = 0;
        double sum = 0.0;
        for (int n = lane(); n < N; n += WAVE) {
            if (c.assoc[n] != m) continue;
            ++call;
            if (c.w[(size_t)m * c.ldn + n] / wmx > 0) { ++cnt; sum += c.langle[n]; }
        }
        cnt = wave_sum_int(cnt);
        call = wave_sum_int(call);
        sum = wave_sum(sum);
        double mean = sum / cnt;
        double sq = 0.0;
        for (int n = lane(); n < N; n += WAVE)
            if (c.assoc[n] == m && c.w[(size_t)m * c.ldn + n] / wmx > 0) {
                double d = c.langle[n] - mean;
                sq += d * d;
            }
        sq = wave_sum(sq);
        if (lane() == 0) {
            sh.err[m] = cnt > 0 ? sqrt(sq / cnt) : __builtin_nan("");   // np.std of an empty set is NaN
            sh.icnt[m] = call;
        }
    }
    block_sync();
    if (c.smoother != 1) {
        // Wave 0, one lane per VP (thread 0's insertion sort through a private array and its serial scan were more than half of
        // the selection: 6.2 of 11.2 CU-ms per YUD batch).  A stable sort puts VP m behind every VP that is smaller and every
        // equal one with a smaller index -- `greater` is the comparison of the sort below --, so each lane counts its own
        // position; the scan's first hit is the lowest set bit of a ballot; the compaction loads four chunks at a time.
        if (wave_id() == 0) {
            int* order = sh.removed;                          // scratch here: every user writes it before it reads it
            for (int m = lane(); m < M; m += WAVE) {
                const double kv = sh.err[m];
                int pos = 0;
                for (int j = 0; j < M; ++j) {
                    const double jv = sh.err[j];
                    const bool j_greater = (is_nan(jv) && !is_nan(kv)) || (jv > kv);
                    const bool m_greater = (is_nan(kv) && !is_nan(jv)) || (kv > jv);
                    pos += (m_greater || (j < m && !j_greater)) ? 1 : 0;
                }
                order[pos] = m;
            }
            wave_sync();
            int worst = -1;
            for (int m0 = 0; m0 < M && worst < 0; m0 += WAVE) {
                const int m = m0 + lane();
                int cand = -1;
                bool ok = false;
                if (m < M) {
                    cand = order[M - 1 - m];
                    const double px = sh.cur[3 * m] / sh.cur[3 * m + 2];    // :557 tests VP m, not worstVPs[m]
                    const double py = sh.cur[3 * m + 1] / sh.cur[3 * m + 2];
                    ok = sh.icnt[cand] > 8 && (px > -1 && py > -1 && px < 1 && py < 1);
                }
                const unsigned long long hits = wave_ballot(ok);
                if (hits) worst = wave_bcast_int(cand, __builtin_ctzll(hits));
            }
            int nw = 0;
            if (worst >= 0)
                for (int n0 = 0; n0 < N; n0 += 4 * WAVE) {
                    int as[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int n = n0 + u * WAVE + lane();
                        as[u] = n < N ? c.assoc[n] : -1;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int n = n0 + u * WAVE + lane();
                        const bool hit = as[u] == worst;      // (worst >= 0; -1 marks a line past the end)
                        const unsigned long long mask = wave_ballot(hit);
                        if (hit) c.idx[nw + popcount64(mask & lanes_below())] = n;
                        nw += popcount64(mask);
                    }
                }
            if (lane() == 0) { sh.ibuf[3] = worst; sh.ibuf[4] = nw; }
        }
        block_sync();
    } else {
        if (tid() == 0) {
            // worstVPs = argsort(stdd)[::-1] (:546-547): ascending with NaN last, reversed
            int order[MAXM];
            for (int m = 0; m < M; ++m) order[m] = m;
            for (int i = 1; i < M; ++i) {                         // stable insertion sort
                int key = order[i];
                double kv = sh.err[key];
                int j = i - 1;
                while (j >= 0) {
                    double jv = sh.err[order[j]];
                    bool greater = (is_nan(jv) && !is_nan(kv)) || (jv > kv);
                    if (!greater) break;
                    order[j + 1] = order[j];
                    --j;
                }
                order[j + 1] = key;
            }
            int worst = -1;
            for (int m = 0; m < M; ++m) {
                int cand = order[M - 1 - m];
                double px = sh.cur[3 * m] / sh.cur[3 * m + 2];    // :557 tests VP m, not worstVPs[m]
                double py = sh.cur[3 * m + 1] / sh.cur[3 * m + 2];
                if (sh.icnt[cand] > 8 && (px > -1 && py > -1 && px < 1 && py < 1)) { worst = cand; break; }
            }
            sh.ibuf[3] = worst;
        }
        block_sync();
        if (wave_id() == 0) {                                     // assocLines, ascending (:552): ordered compaction
            const int worst = sh.ibuf[3];
            int nw = 0;
            if (worst >= 0)
                for (int n0 = 0; n0 < N; n0 += WAVE) {
                    const int n = n0 + lane();
                    const bool hit = n < N && c.assoc[n] == worst;
                    const unsigned long long mask = wave_ballot(hit);
                    if (hit) c.idx[nw + popcount64(mask & lanes_below())] = n;
                    nw += popcount64(mask);
                }
            if (lane() == 0) sh.ibuf[4] = nw;
        }
        block_sync();
    }
    const int worst = sh.ibuf[3], nw = sh.ibuf[4];
    if (tid() == 0) sh.dbuf[11] += lap(tq_);
    if (worst < 0) return 0;
    const double stdd = sh.s[worst] / 2;                      // :566
    gip member = c.idx + N;          // idx has room for 3N ints
    gip csize = c.idx + 2 * N;
    const int ld = nw | 1;
    const bool in_lds = nw <= CLUSTER_LDS_MAX && cluster_lds_doubles(nw) + 3 * nw <= c.wt_doubles;
    double* DL = WT();
    // Ldist (:568-572): 1 - cos(clip(2 acos |cos angle|, -pi/2, pi/2)) for every pair of the set's lines.  The lines'
    // direction vectors and norms are staged in LDS once (not two dependent global loads per pair), and for 2 phi <
    // pi/2 the value is 1 - (2 c^2 - 1) = 2 (1 - c)(1 + c) without acos / cos (as cos9_of_cos does for the similarity:
    // within 2e-16 of the library chain); the clipped branch is numpy's 1 - cos(pi/2) = 1 - 6.123e-17.
    // Staged [nw][vx, vy, norm]: behind the LDS matrix, alone in LDS, or -- a set of more lines than a third of the LDS
    // panel has doubles (3 nw > wt_doubles: thousands of lines on one VP) -- in the slot's p_vl rows in HBM (mcap x ldn >=
    // 8 N doubles; the E-step that follows every split rewrites them before anything reads them).  Same values, same
    // expressions, wherever they are staged.
    const bool dirs_lds = in_lds || 3 * (long long)nw <= c.wt_doubles;
    double* dirs = in_lds ? DL + cluster_lds_doubles(nw) : DL;
    gdp dirs_g = c.pvl;
    for (int a = tid(); a < nw; a += nthreads()) {
        cgdp q = c.lp + 4 * (size_t)c.idx[a];
        const double vx = q[0] - q[2], vy = q[1] - q[3];      // lines_points_cosangle :716-719
        const double nv = norm2(vx, vy);
        if (dirs_lds) { dirs[3 * a] = vx; dirs[3 * a + 1] = vy; dirs[3 * a + 2] = nv; }
        else { dirs_g[3 * (size_t)a] = vx; dirs_g[3 * (size_t)a + 1] = vy; dirs_g[3 * (size_t)a + 2] = nv; }
    }
    block_sync();
    for (long long p = tid(); p < (long long)nw * nw; p += nthreads()) {
        const int a = (int)(p / nw), b = (int)(p - (long long)a * nw);
        double v = 0.0;
        if (a != b) {
            double ax, ay, an, bx, by, bn;
            if (dirs_lds) { ax = dirs[3 * a]; ay = dirs[3 * a + 1]; an = dirs[3 * a + 2]; bx = dirs[3 * b]; by = dirs[3 * b + 1]; bn = dirs[3 * b + 2]; }
            else {
                ax = dirs_g[3 * (size_t)a]; ay = dirs_g[3 * (size_t)a + 1]; an = dirs_g[3 * (size_t)a + 2];
                bx = dirs_g[3 * (size_t)b]; by = dirs_g[3 * (size_t)b + 1]; bn = dirs_g[3 * (size_t)b + 2];
            }
            const double cc = clip(fabs(dot2(ax, ay, bx, by) / (an * bn)), -1.0, 1.0);
            const double COS_PI_4 = 0.70710678118654757;      // cos(pi/4): 2 phi >= pi/2 below it
            if (cc != cc) v = cc;
            else if (!(cc > COS_PI_4)) v = 1 - 6.123233995736766e-17;
            else v = 2 * ((1.0 - cc) * (1.0 + cc));
        }
        // (Ldist is bitwise symmetric, so sklearn's edge test D + D^T != 0 is v + v != 0)
        if (in_lds) DL[a * ld + b] = (a == b || !(v + v != 0.0)) ? -1.0 : v;
        else c.cl[p] = v;
    }
    block_sync();
    if (in_lds) {
        cluster2_lds(nw, c.smoother);
        const int* lmember = cluster_lds_labels(DL, nw);
        for (int q = tid(); q < nw; q += nthreads()) member[q] = lmember[q];
        block_sync();
    } else {
        cluster2(sh, nw, c.cl, member, csize);
    }
    if (tid() == 0) sh.dbuf[12] += lap(tq_);
    // per cluster: smallest right singular vector of the lweight-scaled lines (:580-602)
    // cluster label per line (-1 = not in the set), in the assoc scratch (recomputed before next use)
    gip lab = c.assoc;
    for (int n = tid(); n < N; n += nthreads()) lab[n] = -1;
    block_sync();
    for (int q = tid(); q < nw; q += nthreads()) lab[c.idx[q]] = member[q];
    block_sync();
    for (int cidx = wave_id(); cidx < 2; cidx += nwaves()) {
        int cnt = 0;
        for (int q = lane(); q < nw; q += WAVE) cnt += (member[q] == cidx);
        cnt = wave_sum_int(cnt);
        double vp[3] = {0, 0, 0};
        if (cnt >= 3) {                                       // :592-593
            // rows = lweight * l over the lines of this cluster (:580-595); evaluated over all N lines
            // with weight 0 outside the cluster, so the gather order does not matter
            cgdp lwt = c.lweight;
            wave_null_vector(c.l, N, [=](int n) { return lab[n] == cidx ? lwt[n] : 0.0; }, vp);
        }
        if (lane() == 0) {
            double* o = sh.dbuf + 4 * cidx;
            o[3] = 0.0;
            if (cnt >= 3) {
                if (vp[2] < 0) { vp[0] = -vp[0]; vp[1] = -vp[1]; vp[2] = -vp[2]; }   // :599-600
                o[0] = vp[0]; o[1] = vp[1]; o[2] = vp[2]; o[3] = 1.0;
            }
        }
    }
    block_sync();
    if (tid() == 0) {
        double* v0 = sh.dbuf;
        double* v1 = sh.dbuf + 4;
        bool too_similar = true;                              // :604-615
        if (v0[3] != 0.0 && v1[3] != 0.0) {
            double cphi = clip(dot3(v0[0], v0[1], v0[2], v1[0], v1[1], v1[2]), -1.0, 1.0);
            double ang = fabs(acos(clip(fabs(cphi), -1.0, 1.0)));
            if (ang > c.prm.merge_thresh) too_similar = false;
        }
        sh.ibuf[0] = too_similar ? 0 : SPLIT_WROTE_VPS;
        if (!too_similar) {                                   // :617-628 (both clusters valid here)
            sh.cur[3 * worst] = v0[0]; sh.cur[3 * worst + 1] = v0[1]; sh.cur[3 * worst + 2] = v0[2];
            sh.s[worst] = stdd;
            if (sh.M < MAXM && sh.M < c.mcap) {               // the [vp][line] scratch has mcap rows
                int m = sh.M;
                sh.cur[3 * m] = v1[0]; sh.cur[3 * m + 1] = v1[1]; sh.cur[3 * m + 2] = v1[2];
                sh.nxt[3 * m] = 0; sh.nxt[3 * m + 1] = 0; sh.nxt[3 * m + 2] = 0;
                sh.s[m] = stdd;
                sh.M = m + 1;
            } else {
                sh.flags |= VPK_EM_FLAG_VP_OVERFLOW;
            }
        }
    }
    if (tid() == 0) sh.dbuf[13] += lap(tq_);
    block_sync();
    return sh.ibuf[0] | (dirs_lds ? 0 : SPLIT_WROTE_PVL);     // (ibuf[0]: next written by merge_vps, behind its barriers)
}

}  // namespace vpk
#endif
