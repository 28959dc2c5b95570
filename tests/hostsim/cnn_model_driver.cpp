// cnn_model_driver.cpp -- TEST-ONLY stand-alone program over csrc/cnn_model.hpp: every struct of every layer at the batches of
// tests/test_cnn_model.py, every launch total, the tap tables and the arena, walked in one process with the invariants the kernels
// rely on (tiles cover the layer, totals fit an int, taps stay inside the bordered planes).  Made to be built with the host
// sanitizers and run on its own; it prints one line and returns 0 when every call answered as expected:
//     python tests/hostsim/hostbuild.py drivers
// No test runs it.
#include <limits.h>
#include <stdio.h>

#include "../../vanishing_points_2017_amd/csrc/cnn_model.hpp"

namespace {

int failures = 0, calls = 0;

void expect(bool ok, const char* what) {
    ++calls;
    if (!ok) {
        ++failures;
        printf("FAILED: %s\n", what);
    }
}

bool fits(long long total) { return total > 0 && total <= INT_MAX; }

void batch_all(int B) {
    for (int li = 0; li < 8; ++li) {
        const ConvDims d = at_batch(conv_dims(li), B);
        expect(d.B == B && d.N == B * d.OH * d.OW && d.Kp % BK == 0 && d.Kp >= d.K && d.Mp % TOPO[li].BM == 0 && d.Mp >= d.OC, "ConvDims");
        expect(fits(dma_total(d, TOPO[li].BM)) && dma_total(d, TOPO[li].BM) * DMA_BN * TOPO[li].BM >= (long long)d.groups * d.ksplit * d.N * d.OC,
               "the f32 GEMM's tiles cover the layer");
    }
    const ConvDims f = conv1_fused_at_batch(conv_dims(0), B);
    expect(fits(dma_total(f, 96)) && dma_total(f, 96) == (long long)B * C1B_PATCHES && f.OHp == input_planes(1).Hp && f.opad == 2, "fused conv1");
    for (int group : {1, 3, 4, 64})
        expect(fits(conv1_pieces_total(B, group)) && conv1_pieces_total(B, group) * group >= (long long)B * C1B_PATCHES, "conv1 on pieces");
    expect(fits(conv1_direct_total(B)) && C1_TR * C1_QR >= C1_POOL && C1_TC * C1_QC >= C1_POOL, "conv1 direct");
    for (int li = 1; li <= 4; ++li) {
        const SplitDims sd = at_batch(split_dims(li), B);
        const int blk = blocks_per_tile(li, false);
        expect(sd.mblocks % blk == 0 && sd.mblocks * 32 >= sd.OC && sd.ksteps * 16 == sd.Cg * sd.ntaps, "SplitDims");
        expect(fits(split_total(sd, blk)) && split_total(sd, blk) * SG_BN * blk * 32 >= (long long)sd.groups * sd.N * sd.OC, "the split GEMM's tiles");
        for (bool pairs : {false, true}) {
            PieceDims pd = at_batch(piece_dims(li, pairs), B);
            const int b = blocks_per_tile(li, pairs), rows = piece_tile_rows(li, pairs);
            expect(pd.mblocks == pd.mtiles * b && pd.mblocks * 32 >= pd.OC && pd.rtiles * rows >= pd.OH && (pd.rtiles - 1) * rows < pd.OH &&
                       pd.ctiles * CP_TC >= pd.OW && pd.in_image == (long long)pd.CGtot * (pairs ? 4 : 6) * pd.Hp * pd.Wp * 16, "PieceDims");
            expect(fits(pieces_total(pd)), "the pieces' tiles");
            if (pairs && (li == 2 || li == 3)) {
                hand_planes_to(pd, piece_dims(li + 1, true), 0.5f);
                expect(pd.o_cgtot * 16 == pd.OC * pd.groups && pd.o_Hp == pd.OHp && pd.o_Wp == pd.OWp && pd.o_pad == pd.opad && pd.o_ascale == 0.5f,
                       "the next layer's planes are this layer's output planes");
            }
        }
        if (li == 1) {
            const Wino5Dims w5 = at_batch(wino5_dims(li), B);
            expect(w5.ocblocks * W5_OCB == w5.OC && w5.chunks * W5_KC == w5.IC && fits(wino5_total(w5)), "Wino5Dims");
        } else {
            const WinoDims wd = at_batch(wino_dims(li), B);
            expect(wd.ocblocks * WG_OCB == wd.OC && wd.chunks * WG_KC == wd.IC && fits(wino_total(wd)), "WinoDims");
        }
    }
    for (int li = 5; li <= 6; ++li)
        for (bool pairs : {false, true}) {
            const DenseDims dd = at_batch(dense_dims(li), B, pairs, 8192.f, 0.25f);
            expect(dd.chunks * DP_CHUNK == dd.K && dd.cpp * dd.kparts == dd.chunks && dd.mtiles * DP_BM >= dd.OC && dd.ntiles * DP_BN >= B &&
                       dd.wscale == (pairs ? 8192.f : 1.f) && dd.oscale == (pairs ? 1.f / 2048.f : 1.f) && fits(dense_total(dd)), "DenseDims");
        }
    expect(xfrag_bytes(B) >= (size_t)B * TOPO[5].IC * 6, "fc6's input as three 16-bit pieces");
    expect(fits(norm1_blocks(B)) && fits(norm2_blocks(B)) && fits(pool5_blocks(B)) && pool5_blocks(B) * POOL5_PL >= pool5_planes(B), "pooling grids");
    expect(fits(ew_blocks((long long)B * A_POOL1)) && ew_blocks(1) == 1 && ew_blocks(EW_THREADS + 1) == 2, "element-wise grids");
}

void tables_all() {
    for (int li = 0; li < 5; ++li) {
        const ConvDims d = conv_dims(li);
        const std::vector<unsigned> tab = conv_ktab(li);
        bool inside = (int)tab.size() == d.Kp;
        for (size_t k = 0; k < tab.size(); ++k)
            inside = inside && tab[k] % 4 == 0 && tab[k] / 4 < (unsigned)(d.IC * d.Hp * d.Wp) && (k < (size_t)d.K || tab[k] == 0);
        expect(inside, "a tap table stays inside the layer's planes");
    }
    size_t sum = 0;
    for (int i = 0; i < R_COUNT; ++i) sum += REGION_FLOATS[i];
    expect(sum == arena_floats_per_image() && sum == 8079728, "the arena");
    for (int li = 1; li <= 4; ++li) {
        const Planes p = input_planes(li);
        expect(p.Hp == p.H + 2 * p.pad && p.Wp == p.W + 2 * p.pad && (size_t)p.C * p.Hp * p.Wp == in_planes(li), "bordered planes");
    }
}

}  // namespace

int main() {
    for (int B : {1, 4, 5, 102, 128, 129, 257, MAX_CHUNK}) batch_all(B);
    tables_all();
    printf("cnn_model_driver: %d checks, %d failures\n", calls, failures);
    return failures ? 1 : 0;
}
