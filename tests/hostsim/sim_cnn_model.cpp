// sim_cnn_model.cpp -- TEST-ONLY host build of csrc/cnn_model.hpp (plain C++, no HIP): the kernels' dimension structs per layer and
// per batch, the work items of every launch, the tap table and the arena as flat records for tests/test_cnn_model.py.  Each call
// composes the header's functions the way vpk_cnn.hip does: the struct of the layer, at_batch, the total.
#include "../../vanishing_points_2017_amd/csrc/cnn_model.hpp"

extern "C" {

// out[17]: the fields of ConvDims in declaration order.  fused: conv1's GEMM with the fused epilogue (li = 0)
void sim_conv_dims(int li, int B, int fused, long long* out) {
    const ConvDims d = fused ? conv1_fused_at_batch(conv_dims(li), B) : at_batch(conv_dims(li), B);
    const int v[17] = {d.B, d.IC, d.Hp, d.Wp, d.OC, d.OH, d.OW, d.groups, d.K, d.Kp, d.Mp, d.N, d.ksplit, d.relu, d.OHp, d.OWp, d.opad};
    for (int i = 0; i < 17; ++i) out[i] = v[i];
}

// out[19]: SplitDims in declaration order
void sim_split_dims(int li, int B, long long* out) {
    const SplitDims d = at_batch(split_dims(li), B);
    const int v[19] = {d.B, d.Cg, d.Ctot, d.Hp, d.Wp, d.OC, d.OH, d.OW, d.groups, d.KW, d.ntaps, d.csteps, d.ksteps, d.mblocks, d.N, d.relu,
                       d.OHp, d.OWp, d.opad};
    for (int i = 0; i < 19; ++i) out[i] = v[i];
}

// out[26]: the integer fields of PieceDims in declaration order (in_image at 20; 25: range_word, img_range and live all null);
// fout[2]: o_ascale, oscale.  hand: the epilogue writes layer li + 1's pair planes
void sim_piece_dims(int li, int pairs, int B, int hand, float hscale, float ascale, float next_ascale, long long* out, double* fout) {
    PieceDims d = at_batch(piece_dims(li, pairs != 0), B);
    if (hand) hand_planes_to(d, piece_dims(li + 1, true), next_ascale);
    if (pairs) d.oscale = pair_oscale(hscale, ascale);
    const long long v[26] = {d.B, d.Cg16, d.CGtot, d.Hp, d.Wp, d.OC, d.OH, d.OW, d.groups, d.KW, d.ntaps, d.ksteps, d.mblocks, d.mtiles, d.rtiles,
                             d.ctiles, d.relu, d.OHp, d.OWp, d.opad, d.in_image, d.o_cgtot, d.o_Hp, d.o_Wp, d.o_pad,
                             !d.range_word && !d.range_bit && !d.img_range && !d.live};
    for (int i = 0; i < 26; ++i) out[i] = v[i];
    fout[0] = d.o_ascale; fout[1] = d.oscale;
}

// out[12]: WinoDims in declaration order (conv3..5)
void sim_wino_dims(int li, int B, long long* out) {
    const WinoDims d = at_batch(wino_dims(li), B);
    const int v[12] = {d.IC, d.OC, d.groups, d.ctot_in, d.ctot_out, d.tiles, d.ocblocks, d.chunks, d.OHp, d.OWp, d.opad, d.relu};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
}

// out[9]: Wino5Dims in declaration order (conv2)
void sim_wino5_dims(int li, int B, long long* out) {
    const Wino5Dims d = at_batch(wino5_dims(li), B);
    const int v[9] = {d.IC, d.OC, d.groups, d.ctot_in, d.ctot_out, d.tiles, d.ocblocks, d.chunks, d.relu};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
}

// out[9]: N, K, OC, chunks, kparts, cpp, mtiles, ntiles, live == null; fout[2]: wscale, oscale (fc6, fc7)
void sim_dense_dims(int li, int B, int pairs, float hscale, float ascale, long long* out, double* fout) {
    const DenseDims d = at_batch(dense_dims(li), B, pairs != 0, hscale, ascale);
    const int v[9] = {d.N, d.K, d.OC, d.chunks, d.kparts, d.cpp, d.mtiles, d.ntiles, d.live == nullptr};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
    fout[0] = d.wscale; fout[1] = d.oscale;
}

// The work items (workgroups, for the grids without a tile queue) of a launch of run_forward.  kind:
//   0 conv_gemm_dma_kernel for layer li with BM = arg rows per tile      1 ... conv1 with the fused epilogue
//   2 conv1_pieces_kernel, arg = conv1_group                             3 conv1_direct_kernel
//   4 conv_gemm_split_kernel                                             5 the Winograd kernel of layer li
//   6 conv_pieces_kernel, arg = on fp16 pairs                            7 the dense pieces kernels (fc6, fc7)
//   8 norm1 + pool1 (tiled)     9 norm2 + pool2     10 pool5     11 pool5's planes     12 the bytes of fc6's input fragments
long long sim_total(int kind, int li, int B, int arg) {
    switch (kind) {
    case 0: return dma_total(at_batch(conv_dims(li), B), arg);
    case 1: return dma_total(conv1_fused_at_batch(conv_dims(0), B), 96);
    case 2: return conv1_pieces_total(B, arg);
    case 3: return conv1_direct_total(B);
    case 4: return split_total(at_batch(split_dims(li), B), blocks_per_tile(li, false));
    case 5: return li == 1 ? wino5_total(at_batch(wino5_dims(li), B)) : wino_total(at_batch(wino_dims(li), B));
    case 6: return pieces_total(at_batch(piece_dims(li, arg != 0), B));
    case 7: return dense_total(at_batch(dense_dims(li), B, false, 1.f, 1.f));
    case 8: return norm1_blocks(B);
    case 9: return norm2_blocks(B);
    case 10: return pool5_blocks(B);
    case 11: return pool5_planes(B);
    case 12: return (long long)xfrag_bytes(B);
    }
    return -1;
}
long long sim_ew_blocks(long long n) { return ew_blocks(n); }

// the tap table of conv layer li into out (at most cap entries); returns its length
int sim_ktab(int li, unsigned* out, int cap) {
    const std::vector<unsigned> t = conv_ktab(li);
    for (size_t i = 0; i < t.size() && (int)i < cap; ++i) out[i] = t[i];
    return (int)t.size();
}

// out[6]: C, H, W, Hp, Wp, pad of the bordered planes that layer li reads
void sim_input_planes(int li, long long* out) {
    const Planes p = input_planes(li);
    const int v[6] = {p.C, p.H, p.W, p.Hp, p.Wp, p.pad};
    for (int i = 0; i < 6; ++i) out[i] = v[i];
}

// out[0] = number of regions, then their floats per image; returns the arena's floats per image
long long sim_regions(long long* out) {
    out[0] = R_COUNT;
    for (int i = 0; i < R_COUNT; ++i) out[1 + i] = (long long)REGION_FLOATS[i];
    return (long long)arena_floats_per_image();
}
// out[11]: the floats per image of taps 0 .. 10; out[11], out[12]: the pixels of an image, the outputs per image; out[13]: MAX_CHUNK
void sim_taps(long long* out) {
    for (int i = 0; i < 11; ++i) out[i] = (long long)TAP_FLOATS[i];
    out[11] = (long long)IMAGE_PIXELS; out[12] = (long long)OUTPUTS_PER_IMAGE; out[13] = MAX_CHUNK;
}

}  // extern "C"
