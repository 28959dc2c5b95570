// cnn_topology.hpp -- the static shape of cnn/deploy.prototxt and of the activation arena: host-only constexpr, no HIP.
#ifndef VPK_CNN_TOPOLOGY_HPP_
#define VPK_CNN_TOPOLOGY_HPP_

#include <stddef.h>

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

}  // namespace
#endif
