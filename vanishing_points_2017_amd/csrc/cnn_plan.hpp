// cnn_plan.hpp -- which kernel computes which stage of a CNN forward, and in what format it hands its result on.
//
// cnn_resolve_plan is the ONE place where the arithmetic knobs of include/vpk.h (vpk_cnn_set_precision / _algorithm / _fusion),
// the tap, the image type and the device-counted recompute pass meet; run_forward (vpk_cnn.hip) walks the plan it returns and
// decides nothing itself.  Plain host C++17, no HIP header: tests/hostsim/sim_cnn_plan.cpp compiles it with g++ and
// tests/test_cnn_plan.py checks every combination against the rules as vpk.h words them.
#ifndef VPK_CNN_PLAN_HPP_
#define VPK_CNN_PLAN_HPP_

#include "../../include/vpk.h"

// The knobs of a forward.  vpk_cnn_state keeps one as the user's setting; the calibration forwards and the exact recompute pass
// run on a copy with their own arithmetic.
struct CnnConfig {
    int precision = 0;        // vpk_cnn_set_precision: 0 = f32-input matrix instructions, 1 = conv2..5 as bf16 triples in the split GEMM
    int split_variant = 0;    // ... its modes 2, 3 (development): 1, 2 = force one tiling of the split GEMM for every layer; 0 = per layer
    int algorithm = 4;        // vpk_cnn_set_algorithm (precision 0): 4 = fp16 pairs (default), 2 = exact bf16 triples + Winograd,
                              // 1 = Winograd, 0 = direct f32, 3 = measurements
    int fusion = 3;           // vpk_cnn_set_fusion: conv1 + norm1 + pool1 as 0 = separate kernels, 1 = direct f32, 2 = GEMM-fused,
                              // 3 (default) = exact bf16 pieces, 4 = scaled fp16 pairs
    int conv1_group = 4;      // images per work item of conv1_pieces_kernel (VPK_CONV1_GROUP: development knob)
    int dense_presplit = 1;   // fc6 / fc7 on fp16 pairs: stream the pre-split fragments (VPK_DENSE_PRESPLIT=0: split the f32 stream in registers)
    bool profiling = false;   // vpk_cnn_set_profiling: HIP events between the stages
};

// vpk_cnn_set_precision's mode 0 .. 3 as the two fields it sets
inline void cnn_config_set_precision(CnnConfig& c, int mode) {
    c.precision = mode ? 1 : 0;
    c.split_variant = mode > 1 ? mode - 1 : 0;
}

enum class Conv1Impl { GEMM, DIRECT_F32, GEMM_FUSED, PIECES3, PIECES2 };    // GEMM: followed by the separate LRN / pooling kernel
enum class ConvImpl { DMA_F32, SPLIT_GEMM, WINOGRAD, PIECES3, PIECES2 };    // WINOGRAD: F(2 x 2, 5 x 5) for conv2, F(2 x 2, 3 x 3) for conv3..5
enum class DenseImpl { DMA_F32, PIECES3, PIECES2_STREAMED, PIECES2_PRESPLIT };

struct ConvStage {
    ConvImpl impl = ConvImpl::DMA_F32;
    int split_tiling = 0;             // SPLIT_GEMM: 1 = two 4-wave workgroups per CU, 0 = one 8-wave workgroup (conv4 has one tiling only)
    bool chained_in = false;          // SPLIT_GEMM: the input already is in split format, written by the previous layer
    bool chained_out = false;         // SPLIT_GEMM: write the next layer's split format instead of the f32 blob
    bool needs_to_planes = false;     // PIECES: the f32 input blob is converted to piece planes first (to_planes_kernel)
    bool writes_next_planes = false;  // PIECES2: the epilogue writes the next layer's piece planes instead of the f32 blob
};

struct CnnPlan {
    int err = VPK_OK;                 // VPK_ERR_STATE: the combination is refused (msg says why); nothing else is valid then
    const char* msg = nullptr;
    bool prep_input = false;          // the rasters are first written as f32 phase planes (the GEMM forms of conv1 read those)
    Conv1Impl conv1 = Conv1Impl::PIECES3;
    bool conv1_hands_planes = false;  // its pooling stage writes conv2's piece planes itself (no f32 pool1 blob)
    ConvStage conv[4];                // conv2 .. conv5
    bool norm2_planes = false;        // norm2 + pool2 by lrn5_pool3s2_planes_kernel (else the f32 stream kernel) ...
    bool norm2_hands_planes = false;  // ... which writes conv3's piece planes instead of the f32 pool2 blob
    DenseImpl fc[3] = {DenseImpl::DMA_F32, DenseImpl::DMA_F32, DenseImpl::DMA_F32};   // fc6 .. fc8
};

// tap: -1 = none, 0 .. 10 = the blob vpk_cnn_forward_tap returns (a tapped blob is always written as f32 and converted for the
// layer that reads it).  device_counted: the recompute pass, whose kernels read the number of images from the device.
inline CnnPlan cnn_resolve_plan(const CnnConfig& c, int tap, bool f32_images, bool device_counted) {
    CnnPlan p;
    const bool f32_mfma = c.precision == 0;                      // vpk_cnn_set_algorithm only applies then
    const bool pairs = f32_mfma && c.algorithm == 4;             // conv2..5, fc6, fc7 on scaled fp16 pairs
    const bool triples = f32_mfma && c.algorithm >= 2 && !pairs; // conv2 and fc6 (algorithm 3: conv3 and conv5 too) on exact bf16 triples
    const bool wino = f32_mfma && c.algorithm >= 1;              // Winograd for the layers that are not on pieces
    const bool split = c.precision == 1;

    // conv1: tap 0 needs the conv1 blob, which only the unfused form writes
    if (tap == 0 || c.fusion == 0) p.conv1 = Conv1Impl::GEMM;
    else if (c.fusion == 1) p.conv1 = Conv1Impl::DIRECT_F32;
    else if (c.fusion == 2) p.conv1 = Conv1Impl::GEMM_FUSED;
    else p.conv1 = c.fusion == 4 ? Conv1Impl::PIECES2 : Conv1Impl::PIECES3;
    p.prep_input = p.conv1 == Conv1Impl::GEMM || p.conv1 == Conv1Impl::GEMM_FUSED;
    const bool conv1_pieces = p.conv1 == Conv1Impl::PIECES3 || p.conv1 == Conv1Impl::PIECES2;
    p.conv1_hands_planes = conv1_pieces && pairs && tap != 1;
    // (the scaled fp16-pair conv1 relies on a pixel being an exact fp16 number: uint8 rasters only)
    if (f32_images && p.conv1 == Conv1Impl::PIECES2) {
        p.err = VPK_ERR_STATE;
        p.msg = "vpk_cnn_forward_f32: vpk_cnn_set_fusion(4) takes uint8 rasters only";
    }

    // conv2 .. conv5
    const ConvImpl pieces = pairs ? ConvImpl::PIECES2 : ConvImpl::PIECES3;
    const ConvImpl other = split ? ConvImpl::SPLIT_GEMM : (wino ? ConvImpl::WINOGRAD : ConvImpl::DMA_F32);
    const bool pieces35 = pairs || (triples && c.algorithm == 3);         // conv3 and conv5 on pieces
    p.conv[0].impl = pairs || triples ? pieces : other;
    p.conv[1].impl = pieces35 ? pieces : other;
    p.conv[2].impl = pairs ? pieces : other;
    p.conv[3].impl = pieces35 ? pieces : other;
    p.norm2_planes = pairs;
    p.norm2_hands_planes = pairs && tap != 3;
    // fp16 pairs: conv3 -> conv4 -> conv5 hand over piece planes unless the f32 blob in between is tapped
    p.conv[1].writes_next_planes = pairs && tap != 4;
    p.conv[2].writes_next_planes = pairs && tap != 5;
    p.conv[0].needs_to_planes = (pairs || triples) && !p.conv1_hands_planes;
    p.conv[1].needs_to_planes = pieces35 && !p.norm2_hands_planes;
    p.conv[2].needs_to_planes = pairs && !p.conv[1].writes_next_planes;
    p.conv[3].needs_to_planes = pieces35 && !p.conv[2].writes_next_planes;
    // split precision: conv3 -> conv4 -> conv5 hand over the split format unless a caller taps conv3 or conv4
    const bool chain = split && tap != 4 && tap != 5;
    p.conv[1].chained_out = p.conv[2].chained_in = p.conv[2].chained_out = p.conv[3].chained_in = chain;
    // measured at B = 102 (ms incl. the split pass): conv2 1.10 / conv3 0.82 with two 4-wave workgroups per CU, 1.21 / 0.90
    // with one 8-wave workgroup; conv5 (718 tiles) 0.53 with 8 waves, 0.62 with 4
    for (int i = 0; i < 4; ++i) p.conv[i].split_tiling = c.split_variant == 0 ? (i <= 1 ? 1 : 0) : c.split_variant - 1;

    // fc6 on pieces with conv2; fp16 pairs: fc7 too (fc8's 400 outputs are two row tiles: 0.038 ms against 0.030 on the f32 path)
    const DenseImpl dense2 = c.dense_presplit ? DenseImpl::PIECES2_PRESPLIT : DenseImpl::PIECES2_STREAMED;
    if (pairs) p.fc[0] = p.fc[1] = dense2;
    else if (triples) p.fc[0] = DenseImpl::PIECES3;

    // A device-counted pass: every stage must be a kernel that reads the count -- conv1_pieces_kernel<3>, to_planes / conv_pieces
    // on triples, conv3x3_winograd_kernel, the f32 norm2 stream, pool5, dense_pieces<3> and the dense f32 GEMM; taps copy and
    // events time whole batches.  That is algorithm 2 with the default conv1.
    if (device_counted) {
        const bool counted = p.conv1 == Conv1Impl::PIECES3 && p.conv[0].impl == ConvImpl::PIECES3 &&
                             p.conv[1].impl == ConvImpl::WINOGRAD && p.conv[2].impl == ConvImpl::WINOGRAD &&
                             p.conv[3].impl == ConvImpl::WINOGRAD && !p.norm2_planes && p.fc[0] == DenseImpl::PIECES3 &&
                             p.fc[1] == DenseImpl::DMA_F32 && p.fc[2] == DenseImpl::DMA_F32 && tap < 0 && !c.profiling;
        if (!counted) {           // (checked first by the forward: it outranks the image-type error above)
            p.err = VPK_ERR_STATE;
            p.msg = "run_forward: a device-counted pass runs algorithm 2 with the default conv1, untapped";
        }
    }
    return p;
}

#endif
