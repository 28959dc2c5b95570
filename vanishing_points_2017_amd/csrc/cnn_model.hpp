// cnn_model.hpp -- every number the CNN driver decides on the host: the static shape of cnn/deploy.prototxt, the activation
// arena, the parameter structs the kernels take by value with the tile constants that size them, each struct for layer li
// and for a batch, the work-item total of every launch, and the im2col tap table.  Plain host C++17, no HIP header:
// vpk_cnn.hip and the kernel headers include it, tests/hostsim/sim_cnn_model.cpp compiles it with g++ and
// tests/test_cnn_model.py checks every value against deploy.prototxt's arithmetic.
#ifndef VPK_CNN_MODEL_HPP_
#define VPK_CNN_MODEL_HPP_

#include <stddef.h>

#include <vector>

namespace {

// ---- tile constants (what they mean to a kernel: the header named) ------------------------------------------------------------------
constexpr int BK = 16;                             // cnn_gemm_f32.hpp: K depth of one LDS stage
// conv1 + norm1 + pool1 as ONE kernel: a tile's 128 columns are a 2-D patch of 7 x 17 conv1 outputs (cnn_gemm_f32.hpp, C1FUSE)
constexpr int C1_PR = 7, C1_PC = 17;               // conv outputs per patch (rows x cols): 119 of the tile's 128 columns
constexpr int C1_QR = 3, C1_QC = 8;                // pooled outputs per patch
constexpr int C1_OUT = 123, C1_POOL = 61;          // conv1 / pool1 output size (deploy.prototxt:9-55)
constexpr int C1_TR = (C1_POOL + C1_QR - 1) / C1_QR, C1_TC = (C1_POOL + C1_QC - 1) / C1_QC;   // 21 x 8 patches per image
constexpr int C1_LD = 129;                         // row stride of the patch in LDS ([channel][column])
constexpr int C1_PH = 4, C1_PW = 125;              // conv1 reads its input as 4 x 4 stride-4 phase planes of 125 x 125 (prep_input_kernel)
constexpr int C1B_PATCHES = C1_TR * C1_TC;         // cnn_conv1_pieces.hpp: 168 patch positions per image
constexpr int DMA_BN = 128;                        // cnn_gemm_f32.hpp: columns of a tile (WAVES_N x TN x 32 in every instantiation)
constexpr int SG_BN = 256;                         // cnn_split_gemm.hpp: columns per tile: 8 blocks of 32
constexpr int CP_TC = 32;                          // cnn_conv_pieces.hpp: columns of a tile (its rows: the kernel's NB) ...
constexpr int CP_NB = 4;                           // ... NB as the driver instantiates it: rows of a wave's four 32 x 32 blocks
constexpr int WG_TB = 64;                          // cnn_winograd.hpp, F(2 x 2, 3 x 3): tiles (of 2 x 2 outputs) per workgroup tile
constexpr int WG_OCB = 64;                         // output channels per workgroup tile
constexpr int WG_KC = 8;                           // input channels per LDS stage
constexpr int WG_TILES_PER_IMAGE = 15 * 15;
constexpr int W5_TB = 30;                          // F(2 x 2, 5 x 5): tiles per workgroup tile (of the 32 columns of an MFMA tile: see the transform's lane map)
constexpr int W5_OCB = 64;
constexpr int W5_KC = 4;
constexpr int W5_TPI = 31 * 31;                    // tiles per image (61 x 61 outputs)
constexpr int DP_BM = 256, DP_BN = 128;            // cnn_dense_pieces.hpp: rows (outputs) x columns (images) of a tile
constexpr int DP_CHUNK = 32;                       // k per chunk = two K16 steps
template <int NP> constexpr int DP_STAGE = NP * 2 * 4 * 1024;   // bytes of one chunk's B fragments: [piece][step][column block][lane][8]
constexpr int DP_KPARTS[2] = {45, 16};             // split-K parts of fc6 / fc7 on pieces: work items = 16 row tiles x 45 / 16 K parts
constexpr int LRN_CCH = 16;                        // cnn_norm_pool.hpp: channels per workgroup (plus a 2-channel halo on each side)
constexpr int N1_TPH = 7, N1_TPW = 16;             // norm1 + pool1, tiled kernel: pooled rows x columns per workgroup
constexpr int N2_TPH = 6, N2_CGROUPS = 8;          // norm2 + pool2, stream / planes kernels: pooled rows per workgroup, channel ranges per image
constexpr int POOL5_PL = 8;                        // pool5_kernel: planes per workgroup
constexpr int EW_THREADS = 256;                    // the element-wise kernels: one thread per element

// ---- the parameter structs of the kernels (by value: field order and types are the kernels' argument layout) ------------------------
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

struct SplitDims {
    int B, Cg, Ctot, Hp, Wp;        // input: channels per group / in total; padded plane
    int OC, OH, OW, groups;         // OC = output channels per group
    int KW, ntaps, csteps, ksteps;  // kernel width; KH * KW; K16 steps per tap (Cg / 16); K16 steps in total (ntaps * csteps)
    int mblocks;                    // 32-row blocks per group in the packed weights
    int N;                          // B * OH * OW
    int relu;
    int OHp, OWp, opad;             // f32 NCHW output planes
};

struct PieceDims {
    int B;                                      // images
    int Cg16, CGtot, Hp, Wp;                    // input: channel groups (of 16) per conv group / in the tensor; padded plane
    int OC, OH, OW, groups;                     // OC = output channels per conv group
    int KW, ntaps, ksteps;                      // kernel width; KH * KW; K16 steps per conv group (Cg16 * ntaps)
    int mblocks;                                // 32-row blocks per conv group in the packed weights
    int mtiles, rtiles, ctiles;                 // tiles per (image, conv group): output-channel tiles, row tiles, column tiles
    int relu;
    int OHp, OWp, opad;                         // f32 NCHW output planes
    long long in_image;                         // bytes per image of the input tensor (planes of 16-byte words)
    int o_cgtot, o_Hp, o_Wp, o_pad;             // the NEXT layer's piece planes (written instead of the f32 planes when the kernel gets them)
    float o_ascale;                             //   and its activation scale
    unsigned* range_word;                       //   and where an activation beyond fp16's range is reported (split2h_guard), as bit
    unsigned range_bit;                         //   range_bit (the consuming layer's)
    unsigned* img_range;                        //   and into the image's word of the forward's per-image flags (null: not kept)
    const int* live;                            // recompute pass (vpk_cnn_set_range_policy): the device count of images, B is its upper bound
    float oscale;                               // 1 / (weight scale x activation scale) of the fp16-pair operands (a power of two); 1 for bf16 pieces
};

struct WinoDims {
    int IC, OC, groups;              // channels per group
    int ctot_in, ctot_out;           // channels of the input / output blob
    int tiles;                       // B * 225
    int ocblocks;                    // OC / 64 per group
    int chunks;                      // IC / 8
    int OHp, OWp, opad;              // output planes: (oh, ow) at (oh + opad, ow + opad) of an OHp x OWp plane
    int relu;
};

struct Wino5Dims {
    int IC, OC, groups, ctot_in, ctot_out;
    int tiles;                       // B * 961
    int ocblocks, chunks;
    int relu;
};

struct DenseDims {
    int N, K, OC;                               // images, inputs, outputs
    int chunks, kparts, cpp;                    // K / 32; split-K parts; chunks per part
    int mtiles, ntiles;
    float wscale, oscale;                       // fp16 pairs (NP = 2): weights x wscale before the split; partials x oscale (powers of two)
    const int* live = nullptr;                  // recompute pass (vpk_cnn_set_range_policy): the device count of images, N its upper bound
};

// ---- static topology of cnn/deploy.prototxt (per-group channel counts) --------------------------------------------------------------
// H, W = unpadded input plane, P = convolution padding (the input planes are stored with that zero border), OP = border of the
// OUTPUT planes (= padding of the layer that consumes them; 0 = dense), BM = rows of the f32 GEMM's tile.
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

// floats per image of layer li's input blob with the layer's own zero border / dense, and of its output blob with the consumer's / dense
constexpr size_t in_planes(int li) { return (size_t)TOPO[li].IC * TOPO[li].G * (TOPO[li].H + 2 * TOPO[li].P) * (TOPO[li].W + 2 * TOPO[li].P); }
constexpr size_t in_dense(int li) { return (size_t)TOPO[li].IC * TOPO[li].G * TOPO[li].H * TOPO[li].W; }
constexpr size_t out_planes(int li) { return (size_t)TOPO[li].OC * TOPO[li].G * (TOPO[li].OH + 2 * TOPO[li].OP) * (TOPO[li].OW + 2 * TOPO[li].OP); }
constexpr size_t out_dense(int li) { return (size_t)TOPO[li].OC * TOPO[li].G * TOPO[li].OH * TOPO[li].OW; }
constexpr size_t IMAGE_PIXELS = in_dense(0);            // a raster / float image
constexpr size_t OUTPUTS_PER_IMAGE = out_dense(7);      // the 20 x 20 response map
static_assert(IMAGE_PIXELS == 250000 && OUTPUTS_PER_IMAGE == 400, "500 x 500 pixels in, 400 responses out");

// Activation arena: one region per blob, floats per image.  Regions are carved by the CAPACITY batch,
// so an image's planes sit at the same address for every batch size <= capacity and the zero borders
// written at allocation time stay valid.  Nothing is reused between layers (8 079 728 floats = 32.3 MB per image; 288 GB
// of HBM3E makes ping-pong buffers unnecessary, and the borders must not be overwritten).
enum Region { R_IN, R_CONV1, R_POOL1, R_CONV2, R_POOL2, R_CONV3, R_CONV4, R_CONV5, R_POOL5, R_FCA, R_FCB, R_PART, R_SPLIT, R_SPLIT4, R_SPLIT5, R_P6_2, R_P6_3, R_P6_5, R_COUNT };
constexpr int MAX_CHUNK = 4096;     // images per run_forward at most (32-bit positions inside one launch)
constexpr size_t CTR_FLOATS = 64;   // tile-queue counters of the 8 GEMM launches, behind the regions
constexpr size_t GUARD_FLOATS = 64;  // between the last region and the counters: conv_pieces_kernel's patch DMA reads up to 8 words (128
                                     // bytes) past a plane's last row (columns that are never stored); for the last plane of the last
                                     // image of the last region that must be zeros of the arena, not live counters
static_assert(GUARD_FLOATS * sizeof(float) >= 8 * 16, "the patch DMA's overrun: 8 words of 16 bytes");
constexpr size_t REGION_FLOATS[R_COUNT] = {
    IMAGE_PIXELS,            // fp32 input (raster - mean)
    out_dense(0),            // conv1, dense
    in_planes(1),            // pool1 with conv2's border of 2
    out_dense(1),            // conv2, dense
    in_planes(2),            // pool2 with conv3's border of 1
    out_planes(2),           // conv3 with conv4's border
    out_planes(3),           // conv4 with conv5's border
    out_dense(4),            // conv5, dense
    in_dense(5),             // pool5 = fc6 input
    out_dense(5), out_dense(6),    // fc6 / fc7 outputs
    splitk_partials_per_image(),   // split-K partials (fc6: 72 x 4096 floats = 1.2 MB per capacity image)
    in_planes(1) * 3 / 2,    // the current conv layer's input as three bf16 NHWC pieces (largest: pool1)
    in_planes(3) * 3 / 2,    // conv4's / conv5's input in that format, written by the previous layer's epilogue (interior
    in_planes(4) * 3 / 2,    //  only: the zero border comes from the arena's allocation)
    in_planes(1) * 3 / 2,    // conv2's input as P6 planes (cnn_conv_pieces.hpp: [channel group][piece x k half][y][x] 16-byte words)
    in_planes(2) * 3 / 2,    // conv3's (vpk_cnn_set_algorithm(3) only: measurements)
    in_planes(4) * 3 / 2,    // conv5's (vpk_cnn_set_algorithm(3) only: measurements)
};
static_assert(REGION_FLOATS[R_IN] == 500ull * 500 && REGION_FLOATS[R_CONV1] == 96ull * 123 * 123 && REGION_FLOATS[R_POOL1] == 96ull * 65 * 65 &&
              REGION_FLOATS[R_CONV2] == 256ull * 61 * 61 && REGION_FLOATS[R_POOL2] == 256ull * 32 * 32 && REGION_FLOATS[R_CONV3] == 384ull * 32 * 32 &&
              REGION_FLOATS[R_CONV4] == 384ull * 32 * 32 && REGION_FLOATS[R_CONV5] == 256ull * 900 && REGION_FLOATS[R_POOL5] == 256ull * 225 &&
              REGION_FLOATS[R_FCA] == 4096 && REGION_FLOATS[R_FCB] == 4096 && REGION_FLOATS[R_PART] == 72ull * 4096 &&
              REGION_FLOATS[R_SPLIT] == 96ull * 65 * 65 * 3 / 2 && REGION_FLOATS[R_SPLIT4] == 384ull * 32 * 32 * 3 / 2 &&
              REGION_FLOATS[R_SPLIT5] == 384ull * 32 * 32 * 3 / 2 && REGION_FLOATS[R_P6_2] == 96ull * 65 * 65 * 3 / 2 &&
              REGION_FLOATS[R_P6_3] == 256ull * 32 * 32 * 3 / 2 && REGION_FLOATS[R_P6_5] == 384ull * 32 * 32 * 3 / 2, "the regions as they were written out");
constexpr size_t arena_floats_per_image() {
    size_t t = 0;
    for (int i = 0; i < R_COUNT; ++i) t += REGION_FLOATS[i];
    return t;
}
static_assert(arena_floats_per_image() == 8079728, "32.3 MB per image");
// dense sizes of the blobs a tap can return: tap 0 .. 10
constexpr size_t A_CONV1 = out_dense(0), A_POOL1 = in_dense(1), A_CONV2 = out_dense(1), A_POOL2 = in_dense(2);
constexpr size_t A_CONV3 = out_dense(2), A_CONV4 = out_dense(3), A_CONV5 = out_dense(4), A_POOL5 = in_dense(5);
constexpr size_t A_FC6 = out_dense(5), A_FC7 = out_dense(6), A_FC8 = out_dense(7);
constexpr size_t TAP_FLOATS[11] = {A_CONV1, A_POOL1, A_CONV2, A_POOL2, A_CONV3, A_CONV4, A_CONV5, A_POOL5, A_FC6, A_FC7, A_FC8};
static_assert(A_CONV1 == 96ull * 123 * 123 && A_POOL1 == 96ull * 61 * 61 && A_CONV2 == 256ull * 61 * 61 && A_POOL2 == 256ull * 30 * 30 &&
              A_CONV3 == 384ull * 900 && A_CONV4 == 384ull * 900 && A_CONV5 == 256ull * 900 && A_POOL5 == 256ull * 225 && A_FC6 == 4096 &&
              A_FC7 == 4096 && A_FC8 == 400, "the taps as they were written out");

// The planes of a blob that layer li reads with its zero border: what a pooling stage writes and what an unpad (tap) reads.
struct Planes { int C, H, W, Hp, Wp, pad; };
constexpr Planes input_planes(int li) {
    return Planes{TOPO[li].IC * TOPO[li].G, TOPO[li].H, TOPO[li].W, TOPO[li].H + 2 * TOPO[li].P, TOPO[li].W + 2 * TOPO[li].P, TOPO[li].P};
}
static_assert(input_planes(1).C == 96 && input_planes(1).H == 61 && input_planes(1).Hp == 65 && input_planes(1).Wp == 65 && input_planes(1).pad == 2, "pool1");
static_assert(input_planes(2).C == 256 && input_planes(2).H == 30 && input_planes(2).Hp == 32 && input_planes(2).Wp == 32 && input_planes(2).pad == 1, "pool2");
static_assert(input_planes(3).C == 384 && input_planes(3).H == 30 && input_planes(3).pad == 1 && input_planes(4).C == 384 && input_planes(4).W == 30 &&
              input_planes(4).pad == 1, "conv3 / conv4 with the next layer's border");
static_assert(TOPO[0].OC == 96 && TOPO[0].OH == 123 && TOPO[1].OC * TOPO[1].G == 256 && TOPO[1].OH == 61 && TOPO[4].OC * TOPO[4].G == 256,
              "what norm1, norm2 and pool5 read");

// ---- the structs of layer li, as far as the model decides them (B, N, tiles = 0: at_batch) -----------------------------------------
constexpr int round_up(int n, int m) { return (n + m - 1) / m * m; }

inline ConvDims conv_dims(int li) {             // every layer, on the f32 GEMM
    const Topo& t = TOPO[li];
    ConvDims d = {};
    d.IC = t.IC; d.Hp = t.H + 2 * t.P; d.Wp = t.W + 2 * t.P; d.OC = t.OC; d.OH = t.OH; d.OW = t.OW; d.groups = t.G;
    d.OHp = t.OH + 2 * t.OP; d.OWp = t.OW + 2 * t.OP; d.opad = t.OP;
    if (li == 0) { d.IC = C1_PH * C1_PH; d.Hp = C1_PW; d.Wp = C1_PW; }   // phase planes (K stays 11 x 11)
    d.K = t.IC * t.KH * t.KH;
    d.Kp = round_up(d.K, BK);
    d.Mp = round_up(t.OC, t.BM);
    d.ksplit = KSPLIT[li];
    d.relu = 1;
    return d;
}

// convolution: byte offset of tap k from the patch origin, in the bordered planes; the K padding (conv1: 121 -> 128) points at
// offset 0 and meets zero weights
inline std::vector<unsigned> conv_ktab(int li) {
    const Topo& t = TOPO[li];
    const ConvDims d = conv_dims(li);
    std::vector<unsigned> tab((size_t)d.Kp, 0u);
    for (int k = 0; k < d.K; ++k) {
        const int ic = k / (t.KH * t.KH), r = k % (t.KH * t.KH), kh = r / t.KH, kw = r % t.KH;
        if (li == 0)   // conv1 reads the stride-4 phase planes written by prep_input_kernel
            tab[(size_t)k] = (unsigned)((((kh % C1_PH) * C1_PH + kw % C1_PH) * C1_PW + kh / C1_PH) * C1_PW + kw / C1_PH) * 4u;
        else
            tab[(size_t)k] = (unsigned)((ic * d.Hp + kh) * d.Wp + kw) * 4u;
    }
    return tab;
}

// 32-row blocks of a conv group's output channels per tile.  Split GEMM and bf16 triples: 6 for conv4's 192 channels, else 4 (128);
// fp16 pairs: conv4 as 64 channels x 8 rows, i.e. 2 blocks and twice the tile rows
constexpr int blocks_per_tile(int li, bool pairs) { return TOPO[li].OC == 192 ? (pairs ? 2 : 6) : 4; }
constexpr int piece_tile_rows(int li, bool pairs) { return TOPO[li].OC == 192 && pairs ? 2 * CP_NB : CP_NB; }

inline SplitDims split_dims(int li) {           // conv2..5 on the split GEMM
    const Topo& t = TOPO[li];
    const ConvDims d = conv_dims(li);
    SplitDims sd = {};
    sd.Cg = t.IC; sd.Ctot = t.IC * t.G; sd.Hp = d.Hp; sd.Wp = d.Wp; sd.OC = t.OC; sd.OH = t.OH; sd.OW = t.OW;
    sd.groups = t.G; sd.KW = t.KH; sd.ntaps = t.KH * t.KH; sd.csteps = t.IC / 16; sd.ksteps = sd.ntaps * sd.csteps;
    sd.mblocks = round_up(t.OC / 32, blocks_per_tile(li, false)); sd.relu = 1; sd.OHp = d.OHp; sd.OWp = d.OWp; sd.opad = d.opad;
    return sd;
}

// conv2..5 as direct convolutions on pieces: exact bf16 triples (six 16-byte words per pixel and 16 channels), or scaled fp16
// pairs (four), which pad their 32-row blocks to their own tiles
inline PieceDims piece_dims(int li, bool pairs) {
    const Topo& t = TOPO[li];
    const ConvDims d = conv_dims(li);
    const int blk = blocks_per_tile(li, pairs);
    PieceDims pd = {};
    pd.Cg16 = t.IC / 16; pd.CGtot = t.IC * t.G / 16; pd.Hp = d.Hp; pd.Wp = d.Wp; pd.OC = t.OC; pd.OH = t.OH; pd.OW = t.OW;
    pd.groups = t.G; pd.KW = t.KH; pd.ntaps = t.KH * t.KH; pd.ksteps = pd.ntaps * pd.Cg16; pd.mblocks = round_up(t.OC / 32, blk);
    pd.mtiles = pd.mblocks / blk; pd.rtiles = (t.OH + piece_tile_rows(li, pairs) - 1) / piece_tile_rows(li, pairs);
    pd.ctiles = (t.OW + CP_TC - 1) / CP_TC; pd.relu = 1;
    pd.OHp = d.OHp; pd.OWp = d.OWp; pd.opad = d.opad;
    pd.in_image = (long long)pd.CGtot * (pairs ? 4 : 6) * d.Hp * d.Wp * 16;
    pd.oscale = 1.f;
    return pd;
}

inline WinoDims wino_dims(int li) {             // conv3..5: F(2 x 2, 3 x 3)
    const Topo& t = TOPO[li];
    WinoDims wd = {};
    wd.IC = t.IC; wd.OC = t.OC; wd.groups = t.G; wd.ctot_in = t.IC * t.G; wd.ctot_out = t.OC * t.G;
    wd.ocblocks = t.OC / WG_OCB; wd.chunks = t.IC / WG_KC; wd.OHp = t.OH + 2 * t.OP; wd.OWp = t.OW + 2 * t.OP; wd.opad = t.OP; wd.relu = 1;
    return wd;
}

inline Wino5Dims wino5_dims(int li) {           // conv2: F(2 x 2, 5 x 5)
    const Topo& t = TOPO[li];
    Wino5Dims w5 = {};
    w5.IC = t.IC; w5.OC = t.OC; w5.groups = t.G; w5.ctot_in = t.IC * t.G; w5.ctot_out = t.OC * t.G;
    w5.ocblocks = t.OC / W5_OCB; w5.chunks = t.IC / W5_KC; w5.relu = 1;
    return w5;
}

inline DenseDims dense_dims(int li) {           // fc6, fc7 on pieces
    DenseDims dd;
    dd.N = 0; dd.K = TOPO[li].IC; dd.OC = TOPO[li].OC; dd.chunks = dd.K / DP_CHUNK;
    dd.kparts = DP_KPARTS[li - 5];
    dd.cpp = dd.chunks / dd.kparts;
    dd.mtiles = (dd.OC + DP_BM - 1) / DP_BM; dd.ntiles = 0;
    dd.wscale = 1.f; dd.oscale = 1.f;
    return dd;
}

// ---- ... and for a forward of B images ---------------------------------------------------------------------------------------------
inline ConvDims at_batch(ConvDims d, int B) { d.B = B; d.N = B * d.OH * d.OW; return d; }
inline ConvDims conv1_fused_at_batch(ConvDims d, int B) {     // conv1's GEMM with the fused epilogue: one 128-column tile per patch,
    const Planes p = input_planes(1);                         // written into pool1's planes
    d.B = B; d.N = B * C1B_PATCHES * DMA_BN;
    d.OHp = p.Hp; d.OWp = p.Wp; d.opad = p.pad;
    return d;
}
inline SplitDims at_batch(SplitDims sd, int B) { sd.B = B; sd.N = B * sd.OH * sd.OW; return sd; }
inline WinoDims at_batch(WinoDims wd, int B) { wd.tiles = B * WG_TILES_PER_IMAGE; return wd; }
inline Wino5Dims at_batch(Wino5Dims w5, int B) { w5.tiles = B * W5_TPI; return w5; }
inline PieceDims at_batch(PieceDims pd, int B) { pd.B = B; return pd; }
// fp16 pairs: what the epilogue multiplies by, from the layer's weight scale and its input's activation scale (powers of two)
inline float pair_oscale(float hscale, float ascale) { return 1.f / (hscale * ascale); }
// the epilogue writes the next layer's pair planes (their border is this layer's output border) instead of the f32 blob
inline void hand_planes_to(PieceDims& pd, const PieceDims& next, float next_ascale) {
    pd.o_cgtot = next.CGtot; pd.o_Hp = next.Hp; pd.o_Wp = next.Wp; pd.o_pad = pd.opad; pd.o_ascale = next_ascale;
}
inline DenseDims at_batch(DenseDims dd, int B, bool pairs, float hscale, float ascale) {
    dd.N = B; dd.ntiles = (B + DP_BN - 1) / DP_BN;
    dd.wscale = pairs ? hscale : 1.f;
    dd.oscale = pairs ? pair_oscale(hscale, ascale) : 1.f;
    return dd;
}
// fc6's input as bf16 B fragments (dense_split_kernel), the largest the dense pieces read: bytes
inline size_t xfrag_bytes(int B) { return (size_t)((B + DP_BN - 1) / DP_BN) * (TOPO[5].IC / DP_CHUNK) * DP_STAGE<3>; }

// ---- work items of every launch (the kernels take them as int: MAX_CHUNK keeps them below 2^31, tests/test_cnn_model.py) -----------
inline long long dma_total(const ConvDims& d, int BM) {       // conv_gemm_dma_kernel: BM x 128 tiles (x split-K parts)
    return (long long)d.groups * d.ksplit * ((d.N + DMA_BN - 1) / DMA_BN) * (d.Mp / BM);
}
inline long long conv1_pieces_total(int B, int group) { return (long long)C1B_PATCHES * ((B + group - 1) / group); }   // `group` images per patch position
inline long long conv1_direct_total(int B) { return (long long)B * C1_TR * C1_TC; }
inline long long split_total(const SplitDims& sd, int blk) {  // blk: the tiling's 32-row blocks (blocks_per_tile)
    return (long long)sd.groups * ((sd.N + SG_BN - 1) / SG_BN) * (sd.mblocks / blk);
}
inline long long wino_total(const WinoDims& wd) { return (long long)wd.groups * wd.ocblocks * ((wd.tiles + WG_TB - 1) / WG_TB); }
inline long long wino5_total(const Wino5Dims& w5) { return (long long)w5.groups * w5.ocblocks * ((w5.tiles + W5_TB - 1) / W5_TB); }
inline long long pieces_total(const PieceDims& pd) { return (long long)pd.groups * pd.B * pd.rtiles * pd.ctiles * pd.mtiles; }
inline long long dense_total(const DenseDims& dd) { return (long long)dd.mtiles * dd.ntiles * dd.kparts; }
// workgroups of the grids that have no tile queue
inline long long norm1_blocks(int B) {                        // lrn5_pool3s2_tiled_kernel<N1_TPH, N1_TPW>
    const Planes p = input_planes(1);
    return (long long)B * ((TOPO[0].OC + LRN_CCH - 1) / LRN_CCH) * ((p.H + N1_TPH - 1) / N1_TPH) * ((p.W + N1_TPW - 1) / N1_TPW);
}
inline long long norm2_blocks(int B) { return (long long)B * ((input_planes(2).H + N2_TPH - 1) / N2_TPH) * N2_CGROUPS; }
inline long long pool5_planes(int B) { return (long long)B * TOPO[4].OC * TOPO[4].G; }
inline long long pool5_blocks(int B) { return (pool5_planes(B) + POOL5_PL - 1) / POOL5_PL; }
inline long long ew_blocks(long long n) { return (n + EW_THREADS - 1) / EW_THREADS; }

}  // namespace
#endif
