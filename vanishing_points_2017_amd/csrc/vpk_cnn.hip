// vpk_cnn.hip -- AlexNet-500 forward (cnn/deploy.prototxt:1-304) as hand-written gfx950 kernels.
//
// Caffe conventions reproduced: cross-correlation, OIHW weights, grouped
// convolution splits input/output channels contiguously, MAX pooling with CEIL output size and
// border-clipped windows, LRN across channels x * (1 + alpha/n * sum x^2)^-beta, InnerProduct
// weight (out,in) over the C*H*W-flattened input, Dropout = identity at TEST, input = uint8
// raster minus the mean blob with no scaling (evaluation.py:34-38).
//
// This file is the driver: the loaded model (Layer, vpk_cnn_state), weight loading, run_forward -- one launch per stage of the plan
// that cnn_plan.hpp resolves from the arithmetic settings -- and the C entry points.  It is the CNN's one translation unit; the
// kernels are included:
//   cnn_prims.hpp           what the matrix-core kernels share below their schedules: vector types, counted wait and LDS-only barrier,
//                           LDS-DMA (with wave_prims.hpp), the persistent tile queue -- and why those are inline asm
//   cnn_gemm_f32.hpp        implicit GEMM on the f32-input matrix cores (every layer's f32 form), split-K reduction, weight panels
//   cnn_conv1_direct.hpp    conv1 + LRN + pool as one f32 kernel
//   cnn_norm_pool.hpp       LRN + pool fused, pool5, conv1's input pre-pass, unpad (taps)
//   cnn_split_gemm.hpp      conv2..5 as implicit GEMMs on exact bf16 triples
//   cnn_conv1_pieces.hpp, cnn_conv_pieces.hpp, cnn_norm_pool_planes.hpp, cnn_dense_pieces.hpp (cnn_pairs.hpp)
//                           the defaults: exact bf16 triples / scaled fp16 pairs of the f32 operands
//   cnn_winograd.hpp        Winograd minimal filtering on the f32-input matrix cores
//   cnn_calibrate.hpp, cnn_range_policy.hpp   activation scales of the fp16 pairs; exact recompute of images that leave their range
// Every number the host decides -- the kernels' dimension structs per layer and per batch, the work items of each launch, the arena -- is
// cnn_model.hpp's, plain C++ that the CPU suite tests; load_model and run_forward ask it, pack, upload and launch.
// Activations live in HBM for the whole batch (cnn_model.hpp: B x 96 x 123 x 123 fp32 is 0.6 GB at B = 102; 288 GB of HBM3E
// makes chunking unnecessary up to B ~ 4000).
#include "vpk_internal.hpp"

#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>

#include "cnn_plan.hpp"
#include "cnn_model.hpp"
#include "cnn_prims.hpp"     // first of the device headers, and here at file scope: it brings wave_prims.hpp and the HIP runtime
#include "cnn_gemm_f32.hpp"
#include "cnn_conv1_direct.hpp"
#include "cnn_norm_pool.hpp"

namespace {

// (these headers open an anonymous namespace of their own; they stay nested in this one so that their kernels keep their symbol names.
//  Each names cnn_prims.hpp, which is already in -- at file scope, above: opened here it would put the HIP runtime's declarations in this namespace)
#include "cnn_split_gemm.hpp"
#include "cnn_pairs.hpp"
#include "cnn_conv1_pieces.hpp"
#include "cnn_conv_pieces.hpp"
#include "cnn_norm_pool_planes.hpp"
#include "cnn_dense_pieces.hpp"
#include "cnn_winograd.hpp"

// a device allocation owned by its holder: move-only, released with it
template <typename T>
struct DeviceBuffer {
    T* p = nullptr;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.p) { o.p = nullptr; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~DeviceBuffer() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; }
    void** out() { return (void**)&p; }     // for hipMalloc / vpk_reserve
    operator T*() const { return p; }
};

// the dimension structs are cnn_model.hpp's for the layer; run_forward copies and patches them per batch
struct Layer {
    ConvDims d;
    DeviceBuffer<float> wp;     // packed weights
    DeviceBuffer<float> bias;
    DeviceBuffer<unsigned> ktab;   // im2col table (conv layers): byte offset of tap k inside the padded input planes
    DeviceBuffer<unsigned short> wsplit;   // conv2..5: weights as three bf16 pieces in MFMA fragment order (cnn_split_gemm.hpp)
    float ascale = CP_DEFAULT_ASCALE;   // conv2..5, fc6, fc7 on fp16 pairs: the power of two the layer's INPUT is multiplied by (calibrate())
    float hscale = 1.f;                 // conv2..5, fc6, fc7: the power of two the weights are multiplied by before the fp16 split (largest in [2^13, 2^14))
    DeviceBuffer<unsigned short> whalf;    // conv2..5: weights as scaled fp16 pairs in the same order (cnn_conv_pieces.hpp, NP = 2)
    PieceDims pdh;                      //            and the layer's dimensions for that path (own block padding)
    SplitDims sd;
    DeviceBuffer<float> wino;   // conv2..5: G g G^T in the chunk order of the Winograd kernels (cnn_winograd.hpp)
    DeviceBuffer<unsigned short> c1frag;   // conv1: three bf16 pieces of every weight in MFMA fragment order (cnn_conv1_pieces.hpp)
    DeviceBuffer<unsigned short> c1half;   // conv1: scaled fp16 pairs in the same order (c1scale: the power of two)
    float c1scale = 1.f;
    DeviceBuffer<float> c1map;  // conv1: bias - conv1(mean), 123 x 123 x 96
    WinoDims wd;
    Wino5Dims wd5;
    PieceDims pd;               // conv2..5 on exact bf16 pieces from an LDS-resident patch (cnn_conv_pieces.hpp)
    DenseDims dd;               // fc6, fc7 on pieces (cnn_dense_pieces.hpp)
    DeviceBuffer<float> wraw;   // fc6, fc7: the f32 weights in tile order (dense_tile_weights_kernel), streamed by dense_pieces_kernel
    DeviceBuffer<unsigned short> wpair;   // fc6, fc7: the same weights as scaled fp16 pairs in A-fragment order (dense_pair_weights_kernel): the default's stream
};

}  // namespace

struct vpk_cnn_state {
    // the loaded model
    Layer L[8];              // conv1..5, fc6..8
    DeviceBuffer<float> mean;
    bool loaded = false;
    // how the layers are computed: the user's setting (vpk_cnn_set_precision / _algorithm / _fusion / _profiling, cnn_plan.hpp)
    CnnConfig cfg;
    // workspaces (grown on demand)
    DeviceBuffer<float> act;           // the activation arena (cnn_model.hpp)
    size_t act_bytes = 0;
    int act_batch = 0;
    DeviceBuffer<unsigned short> xfrag;   // fc6's input as bf16 B fragments (dense_split_kernel)
    size_t xfrag_bytes = 0;
    // value range of the fp16 pairs
    DeviceBuffer<unsigned> range_word; // bit li set when a scaled INPUT value of layer li reached fp16's range (split2h_guard);
                                       // sticky until vpk_cnn_range_flags reads and clears it.  range_word[1]: where the pair pass
                                       // reports under RECOMPUTE_EXACT (its flagged images are recomputed, so nothing reaches word 0)
    int range_policy = 0;              // vpk_cnn_set_range_policy: 0 = RAISE, 1 = RECOMPUTE_EXACT
    DeviceBuffer<unsigned> img_range;  // the last vpk_cnn_forward's per-image bits (image b at [b]), grown on demand
    size_t img_range_bytes = 0;
    int img_range_batch = 0;           // its batch (0: no forward yet)
    DeviceBuffer<int> rc_list;         // recompute pass: [0] = device count of flagged images of the chunk, [1 ..] their indices in order
    DeviceBuffer<unsigned long long> rc_total;   // images recomputed since vpk_cnn_recomputed last read it
    // optional per-layer timing (cfg.profiling): HIP events on the handle's stream
    static constexpr int EV_RING = 64;   // event sets of the last 64 profiled passes (vpk_cnn_mean_layer_ms)
    hipEvent_t ev[EV_RING][14] = {};
    long long ev_pass = 0;   // profiled passes recorded since profiling was switched on
    bool ev_ready = false;
    bool ev_valid = false;
    __attribute__((visibility("hidden"))) ~vpk_cnn_state() = default;   // (only vpk_cnn_free deletes one: not an export of the library)
};

void vpk_cnn_free(vpk_handle* h) {      // (the state's buffers go with it)
    if (!h->cnn) return;
    if (h->cnn->ev_ready)
        for (auto& set : h->cnn->ev)
            for (auto& e : set) (void)hipEventDestroy(e);
    delete h->cnn;
    h->cnn = nullptr;
}

namespace {

template <typename KernelT>
void launch_dma(vpk_handle* h, KernelT kernel, const ConvDims& d, int BM, const float* in, const Layer& l, float* out,
                int stride, int* counter, int wpc = 3, const int* live = nullptr) {
    const long long total = dma_total(d, BM);
    long long blocks = std::min<long long>(total, (long long)wpc * h->num_cu);   // wpc workgroups fit a CU (LDS, registers)
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(CONV_THREADS), 0, h->stream, d, in, l.wp.p, l.bias.p, l.ktab.p,
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
    Images at(size_t b) const { return Images{f32 ? (const void*)(f() + b * IMAGE_PIXELS) : (const void*)(u8() + b * IMAGE_PIXELS), f32}; }
};

// One forward of at most MAX_CHUNK images under `cfg`: the handle's setting, or the arithmetic an internal pass needs (the calibration
// forwards, the exact recompute).  The plan says which kernel runs each stage (cnn_plan.hpp); this function only launches.
int run_forward(vpk_handle* h, const CnnConfig& cfg, Images img, int batch, float* out, int tap, float* tap_out, const FwdCtl& fc) {
    vpk_cnn_state* S = h->cnn;
    hipStream_t st = h->stream;
    const CnnPlan plan = cnn_resolve_plan(cfg, tap, img.f32, fc.live != nullptr);
    if (plan.err) return vpk_fail(h, plan.err, plan.msg);
    const int* live = fc.live;
    if (batch > S->act_batch) {     // grow the arena; all borders (and everything else) start as zeros
        const size_t need = ((size_t)batch * arena_floats_per_image() + GUARD_FLOATS + CTR_FLOATS) * sizeof(float);
        int rc = vpk_reserve(h, S->act.out(), &S->act_bytes, need, "hipMalloc(CNN activations)");
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
    auto tapunpad = [&](int id, const float* src, int li) {       // the bordered planes that layer li reads
        if (tap == id && tap_out) {
            const Planes p = input_planes(li);
            const long long planes = (long long)batch * p.C;
            hipLaunchKernelGGL(unpad_kernel, dim3((unsigned)ew_blocks(planes * p.H * p.W)), dim3(EW_THREADS), 0, st, src, tap_out, planes,
                               p.H, p.W, p.Hp, p.Wp, p.pad);
        }
    };
    auto dims = [&](int li) { return at_batch(S->L[li].d, batch); };
    const Planes pool1 = input_planes(1), pool2 = input_planes(2);
    // profiling: 14 events per pass, one in front of conv1 and one behind each of the 13 slots of vpk_cnn_last_layer_ms (vpk.h);
    // a stage that covers several slots records all of their events when it ends
    int evi = 0;
    hipEvent_t* evs = S->ev[S->ev_pass % vpk_cnn_state::EV_RING];
    auto mark = [&](int slots) {
        for (; cfg.profiling && slots > 0 && evi < 14; --slots) (void)hipEventRecord(evs[evi++], st);
    };
    int rc;
    mark(1);

    // ---- conv1 + relu1 + norm1 + pool1 -> pool1's planes with conv2's border of 2 (slots conv1, norm1, pool1) ----
    if (plan.prep_input) {          // uint8 raster (float image) - mean -> fp32 phase planes for the GEMM forms
        const dim3 grid((unsigned)ew_blocks(IMAGE_PIXELS), batch);
        if (img.f32)
            hipLaunchKernelGGL(prep_input_kernel<float>, grid, dim3(EW_THREADS), 0, st, img.f(), S->mean.p, R[R_IN], (int)IMAGE_PIXELS);
        else
            hipLaunchKernelGGL(prep_input_kernel<unsigned char>, grid, dim3(EW_THREADS), 0, st, img.u8(), S->mean.p, R[R_IN], (int)IMAGE_PIXELS);
    }
    switch (plan.conv1) {
    case Conv1Impl::GEMM:           // separate kernels: the only form that writes the conv1 blob
        launch_dma(h, conv_gemm_dma_kernel<1, 4, 3, 1, false>, dims(0), 96, R[R_IN], S->L[0], R[R_CONV1], 1, ctr + 0);   // stride 1 over the phase planes
        mark(1);
        if ((rc = tapcopy(0, R[R_CONV1], A_CONV1))) return rc;
        hipLaunchKernelGGL((lrn5_pool3s2_tiled_kernel<N1_TPH, N1_TPW>), dim3((unsigned)norm1_blocks(batch)), dim3(256), 0, st, R[R_CONV1],
                           R[R_POOL1], TOPO[0].OC, TOPO[0].OH, TOPO[0].OW, pool1.H, pool1.W, 1e-4f, 0.75f, pool1.Hp, pool1.Wp, pool1.pad);
        mark(2);
        break;
    // the fused forms: 21 x 8 patches of 7 x 17 conv outputs per image, straight into pool1's planes
    case Conv1Impl::PIECES3:        // exact bf16 pieces / scaled fp16 pairs on the matrix cores (cnn_conv1_pieces.hpp)
    case Conv1Impl::PIECES2: {
        const int group = cfg.conv1_group;
        const int total = (int)conv1_pieces_total(batch, group);
        // fp16 pairs downstream and pool1 not tapped: the pooling stage writes conv2's piece planes itself (no f32 pool1 blob)
        unsigned short* c2planes = plan.conv1_hands_planes ? reinterpret_cast<unsigned short*>(R[R_P6_2]) : nullptr;
        if (plan.conv1 == Conv1Impl::PIECES2)
            hipLaunchKernelGGL(conv1_pieces_kernel<2>, dim3((unsigned)std::min(total, h->num_cu)), dim3(C1B_THREADS), 0, st, img.u8(),
                               S->L[0].c1half.p, S->L[0].c1map.p, R[R_POOL1], pool1.Hp, pool1.Wp, pool1.pad, batch, group, 1.f / S->L[0].c1scale, ctr + 0, total,
                               c2planes, S->L[1].ascale, fc.range_word, fc.img_range, live);
        else if (img.f32)               // float images: three pieces per pixel, six products per K step
            hipLaunchKernelGGL((conv1_pieces_kernel<3, float>), dim3((unsigned)std::min(total, h->num_cu)), dim3(C1B_THREADS), 0, st,
                               img.f(), S->L[0].c1frag.p, S->L[0].c1map.p, R[R_POOL1], pool1.Hp, pool1.Wp, pool1.pad, batch, group, 1.f, ctr + 0, total,
                               c2planes, S->L[1].ascale, fc.range_word, fc.img_range, live);
        else
            hipLaunchKernelGGL(conv1_pieces_kernel<3>, dim3((unsigned)std::min(total, h->num_cu)), dim3(C1B_THREADS), 0, st, img.u8(),
                               S->L[0].c1frag.p, S->L[0].c1map.p, R[R_POOL1], pool1.Hp, pool1.Wp, pool1.pad, batch, group, 1.f, ctr + 0, total,
                               c2planes, S->L[1].ascale, fc.range_word, fc.img_range, live);
        mark(3);
        break;
    }
    case Conv1Impl::GEMM_FUSED: {   // the implicit-GEMM kernel with the fused epilogue (kept for comparison)
        launch_dma(h, conv_gemm_dma_kernel<1, 4, 3, 1, false, true>, conv1_fused_at_batch(S->L[0].d, batch), 96, R[R_IN], S->L[0], R[R_POOL1],
                   1, ctr + 0);
        mark(3);
        break;
    }
    case Conv1Impl::DIRECT_F32: {   // reads the rasters itself (cnn_conv1_direct.hpp)
        const int total = (int)conv1_direct_total(batch);
        if (img.f32)
            hipLaunchKernelGGL(conv1_direct_kernel<float>, dim3((unsigned)std::min(total, h->num_cu)), dim3(C1D_THREADS), 0, st, img.f(),
                               S->mean.p, S->L[0].wp.p, S->L[0].bias.p, R[R_POOL1], pool1.Hp, pool1.Wp, pool1.pad, ctr + 0, total);
        else
            hipLaunchKernelGGL(conv1_direct_kernel<unsigned char>, dim3((unsigned)std::min(total, h->num_cu)), dim3(C1D_THREADS), 0, st,
                               img.u8(), S->mean.p, S->L[0].wp.p, S->L[0].bias.p, R[R_POOL1], pool1.Hp, pool1.Wp, pool1.pad, ctr + 0, total);
        mark(3);
        break;
    }
    }
    tapunpad(1, R[R_POOL1], 1);

    // ---- conv2 .. conv5 (+ relu): the launchers of the four forms, then conv_stage picks by the plan ----
    // (a 2-stage / 4-workgroups-per-CU build of the f32 GEMM, NST = 2, WPC = 4, was measured in round 2: conv2 +2 %,
    //  conv3 -3 %, conv5 -11 % (1436 tiles on 1024 workgroups) -- not used)
    // split GEMM (precision 1): the layer's input planes are split into three bf16 NHWC pieces, the GEMM runs on the bf16 matrix cores
    // src_split: the input already is in split format (written by the previous layer); dst_split: write that format
    auto conv_split = [&](int li, int tiling, const float* src, const unsigned short* src_split, void* dst, bool dst_split) {
        const Layer& l = S->L[li];
        const SplitDims sd = at_batch(l.sd, batch);
        const unsigned short* sp = src_split;
        if (!sp) {
            unsigned short* cv = reinterpret_cast<unsigned short*>(R[R_SPLIT]);
            hipLaunchKernelGGL(split_nhwc_kernel, dim3((unsigned)sd.Hp, (unsigned)batch), dim3(256),
                               (size_t)sd.Ctot * (sd.Wp + 1) * sizeof(float), st, src, cv, sd.Ctot, sd.Hp, sd.Wp);
            sp = cv;
        }
        const int total = (int)split_total(sd, blocks_per_tile(li, false));     // 32-row blocks per tile: the kernels' WAVES_M x TM
        auto go = [&](auto kernel, int threads, int per_cu) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)std::min(total, per_cu * h->num_cu)), dim3(threads), 0, st, sd, sp, l.wsplit.p,
                               l.bias.p, dst, ctr + li, total);
        };
        if (sd.OC == 192) {
            if (dst_split) go(conv_gemm_split_kernel<2, 4, 3, 3, 2, true>, 512, 1);
            else go(conv_gemm_split_kernel<2, 4, 3, 3, 2, false>, 512, 1);
        } else if (tiling == 1) {       // two independent 4-wave workgroups per CU, two stages each
            if (dst_split) go(conv_gemm_split_kernel<2, 2, 2, 2, 2, true>, 256, 2);
            else go(conv_gemm_split_kernel<2, 2, 2, 2, 2, false>, 256, 2);
        } else {
            if (dst_split) go(conv_gemm_split_kernel<2, 4, 2, 3, 2, true>, 512, 1);
            else go(conv_gemm_split_kernel<2, 4, 2, 3, 2, false>, 512, 1);
        }
    };
    auto conv_wino = [&](int li, const float* src, float* dst) {      // conv2 by F(2 x 2, 5 x 5), conv3 / conv4 / conv5 by F(2 x 2, 3 x 3)
        if (li == 1) {
            const Wino5Dims w5 = at_batch(S->L[1].wd5, batch);
            const int total = (int)wino5_total(w5);
            hipLaunchKernelGGL(conv5x5_winograd_kernel, dim3((unsigned)std::min(total, h->num_cu)), dim3(W5_THREADS), 0, st, w5, src,
                               S->L[1].wino.p, S->L[1].bias.p, dst, ctr + 1, total);
            return;
        }
        const WinoDims wd = at_batch(S->L[li].wd, batch);
        const int total = (int)wino_total(wd);
        hipLaunchKernelGGL(conv3x3_winograd_kernel, dim3((unsigned)std::min(total, h->num_cu)), dim3(WG_THREADS), 0, st, wd, src,
                           S->L[li].wino.p, S->L[li].bias.p, dst, ctr + li, total, live);
    };
    // direct convolutions on pieces (cnn_conv_pieces.hpp), pairs: scaled fp16 pairs, else exact bf16 triples.  to_p6: layer li's bordered
    // f32 input planes as its piece planes
    auto to_p6 = [&](int li, bool pairs, const float* src, unsigned short* dst) {
        const ConvDims& d = S->L[li].d;
        const int C = d.IC * d.groups;
        if (pairs) hipLaunchKernelGGL(to_planes_kernel<2>, dim3((unsigned)d.Hp, (unsigned)(C / 16), (unsigned)batch), dim3(256), 0, st, src, dst, C, d.Hp, d.Wp,
                                      S->L[li].ascale, fc.range_word, 1u << li, fc.img_range, live);
        else hipLaunchKernelGGL(to_planes_kernel<3>, dim3((unsigned)d.Hp, (unsigned)(C / 16), (unsigned)batch), dim3(256), 0, st, src, dst, C, d.Hp, d.Wp, 1.f,
                                fc.range_word, 0u, nullptr, live);
    };
    // (planes_next: the next layer's input planes, written by the epilogue instead of the f32 blob -- fp16 pairs only)
    auto conv_pieces = [&](int li, bool pairs, const unsigned short* src6, float* dst, unsigned short* planes_next) {
        PieceDims pd = at_batch(pairs ? S->L[li].pdh : S->L[li].pd, batch);
        if (planes_next) hand_planes_to(pd, S->L[li + 1].pdh, S->L[li + 1].ascale);
        pd.range_word = fc.range_word; pd.range_bit = 1u << (li + 1); pd.img_range = fc.img_range; pd.live = live;
        if (pairs) pd.oscale = pair_oscale(S->L[li].hscale, S->L[li].ascale);
        constexpr int nb = CP_NB;                                           // rows of a wave's four 32 x 32 blocks
        const int total = (int)pieces_total(pd);
        const unsigned blocks = (unsigned)std::min(total, 2 * h->num_cu);   // two workgroups per CU (LDS: two patch buffers each)
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(CP_THREADS), 0, st, pd, src6, pairs ? S->L[li].whalf.p : S->L[li].wsplit.p, S->L[li].bias.p,
                               dst, planes_next, ctr + li, total);
        };
        if (pairs) { if (li == 1) go(conv_pieces_kernel<5, nb, 2, 1>); else if (li == 3) go(conv_pieces_kernel<3, nb, 2, 2>); else go(conv_pieces_kernel<3, nb, 2, 1>); }
        else { if (li == 1) go(conv_pieces_kernel<5, nb, 3, 1>); else go(conv_pieces_kernel<3, nb, 3, 1>); }
    };
    // Layer li from its f32 input blob `src` to its f32 blob `dst`, unless the plan says that a neighbour hands over another format:
    // planes / planes_next = the layer's input as piece planes and where its epilogue writes the next layer's; split_in / split_out
    // = the same for the split GEMM's chained format.
    auto conv_stage = [&](int li, const float* src, float* dst, unsigned short* planes, unsigned short* planes_next,
                          const unsigned short* split_in, unsigned short* split_out) {
        const ConvStage& cs = plan.conv[li - 1];
        const bool pairs = cs.impl == ConvImpl::PIECES2;
        switch (cs.impl) {
        case ConvImpl::PIECES3:
        case ConvImpl::PIECES2:
            if (cs.needs_to_planes) to_p6(li, pairs, src, planes);
            conv_pieces(li, pairs, planes, dst, cs.writes_next_planes ? planes_next : nullptr);
            break;
        case ConvImpl::SPLIT_GEMM:
            conv_split(li, cs.split_tiling, src, cs.chained_in ? split_in : nullptr, cs.chained_out ? (void*)split_out : (void*)dst, cs.chained_out);
            break;
        case ConvImpl::WINOGRAD:
            conv_wino(li, src, dst);
            break;
        case ConvImpl::DMA_F32:         // conv4 (2 x 192 channels): 96 x 128 tiles; the others 128 x 128
            if (li == 3) launch_dma(h, conv_gemm_dma_kernel<1, 4, 3, 1, false>, dims(3), 96, src, S->L[3], dst, 1, ctr + 3);
            else launch_dma(h, conv_gemm_dma_kernel<2, 2, 2, 2, false>, dims(li), 128, src, S->L[li], dst, 1, ctr + li);
            break;
        }
    };
    unsigned short* p6_2 = reinterpret_cast<unsigned short*>(R[R_P6_2]);
    unsigned short* p6_3 = reinterpret_cast<unsigned short*>(R[R_P6_3]);
    unsigned short* p6_5 = reinterpret_cast<unsigned short*>(R[R_P6_5]);
    unsigned short* s4 = reinterpret_cast<unsigned short*>(R[R_SPLIT4]);
    unsigned short* s5 = reinterpret_cast<unsigned short*>(R[R_SPLIT5]);
    conv_stage(1, R[R_POOL1], R[R_CONV2], p6_2, nullptr, nullptr, nullptr);
    mark(1);
    if ((rc = tapcopy(2, R[R_CONV2], A_CONV2))) return rc;
    // norm2 + pool2 (fused), written with conv3's border (slots norm2, pool2)
    // (13 rows x 61 columns = 793 pixels per channel and workgroup <= 4 x 256 thread slots; 5 row tiles x 8 channel ranges
    //  of 32 channels per image; measured at B = 102: 0.177 ms against 0.235 ms for lrn5_pool3s2_tiled_kernel<6, 15>)
    if (plan.norm2_planes)          // fp16 pairs: conv3's input planes straight from the pooling stage (cnn_norm_pool_planes.hpp), unless pool2 is tapped
        hipLaunchKernelGGL((lrn5_pool3s2_planes_kernel<N2_TPH>), dim3((unsigned)norm2_blocks(batch)), dim3(256), 0, st, R[R_CONV2], R[R_POOL2],
                           plan.norm2_hands_planes ? p6_3 : nullptr, pool2.C, TOPO[1].OH, TOPO[1].OW, pool2.H, pool2.W, 1e-4f, pool2.Hp, pool2.Wp,
                           pool2.pad, N2_CGROUPS, S->L[2].ascale, fc.range_word, 1u << 2, fc.img_range);
    else
        hipLaunchKernelGGL((lrn5_pool3s2_stream_kernel<N2_TPH, 4>), dim3((unsigned)norm2_blocks(batch)), dim3(256), 0, st, R[R_CONV2], R[R_POOL2],
                           pool2.C, TOPO[1].OH, TOPO[1].OW, pool2.H, pool2.W, 1e-4f, 0.75f, pool2.Hp, pool2.Wp, pool2.pad, N2_CGROUPS, live);
    mark(2);
    tapunpad(3, R[R_POOL2], 2);
    // conv3 -> conv4 -> conv5.  Pieces: conv3's epilogue writes conv4's planes into p6_5, conv4's writes conv5's into p6_3, which conv3
    // has finished reading; the split GEMM chains through s4 and s5.  A tapped f32 blob is written as such and converted for the next layer.
    conv_stage(2, R[R_POOL2], R[R_CONV3], p6_3, p6_5, nullptr, s4);
    mark(1);
    tapunpad(4, R[R_CONV3], 3);
    conv_stage(3, R[R_CONV3], R[R_CONV4], p6_5, p6_3, s4, s5);
    mark(1);
    tapunpad(5, R[R_CONV4], 4);
    conv_stage(4, R[R_CONV4], R[R_CONV5], plan.conv[2].writes_next_planes ? p6_3 : p6_5, nullptr, s5, nullptr);
    mark(1);
    if ((rc = tapcopy(6, R[R_CONV5], A_CONV5))) return rc;
    hipLaunchKernelGGL((pool5_kernel<POOL5_PL>), dim3((unsigned)pool5_blocks(batch)), dim3(256), 0, st, R[R_CONV5], R[R_POOL5],
                       pool5_planes(batch), live);
    mark(1);
    if ((rc = tapcopy(7, R[R_POOL5], A_POOL5))) return rc;

    // ---- fc6 / fc7 / fc8: split-K partials + deterministic reduction (+ bias, ReLU / sigmoid) ----
    float* fc_in = R[R_POOL5];
    float* fc_out = R[R_FCA];
    for (int li = 5; li < 8; ++li) {
        ConvDims d = dims(li);
        const DenseImpl impl = plan.fc[li - 5];
        if (impl == DenseImpl::DMA_F32) {
            launch_dma(h, conv_gemm_dma_kernel<2, 2, 2, 2, true>, d, 128, fc_in, S->L[li], R[R_PART], 1, ctr + li, 3, live);
        } else {
            // on pieces (cnn_dense_pieces.hpp): the input split into B fragments; the weights streamed as f32 in tile order and split in
            // registers -- exact bf16 triples, or scaled fp16 pairs -- or, the pairs' default, streamed pre-split
            const bool pairs = impl != DenseImpl::PIECES3;
            DenseDims dd = at_batch(S->L[li].dd, batch, pairs, S->L[li].hscale, S->L[li].ascale);
            dd.live = live;
            if ((rc = vpk_reserve(h, S->xfrag.out(), &S->xfrag_bytes, xfrag_bytes(batch), "hipMalloc(dense input fragments)"))) return rc;
            const int total = (int)dense_total(dd);
            const dim3 split_grid((unsigned)dd.chunks, (unsigned)dd.ntiles), grid((unsigned)std::min(total, h->num_cu));
            if (pairs)
                hipLaunchKernelGGL(dense_split_kernel<2>, split_grid, dim3(256), 0, st, fc_in, S->xfrag.p, batch,
                                   d.K, dd.chunks, S->L[li].ascale, fc.range_word, 1u << li, fc.img_range, nullptr);
            else
                hipLaunchKernelGGL(dense_split_kernel<3>, split_grid, dim3(256), 0, st, fc_in, S->xfrag.p, batch,
                                   d.K, dd.chunks, 1.f, fc.range_word, 0u, nullptr, live);
            switch (impl) {
            case DenseImpl::PIECES2_PRESPLIT:
                hipLaunchKernelGGL(dense_pairs_kernel, grid, dim3(DP_THREADS), 0, st, dd, S->L[li].wpair.p, S->xfrag.p, R[R_PART], ctr + li, total);
                break;
            case DenseImpl::PIECES2_STREAMED:
                hipLaunchKernelGGL(dense_pieces_kernel<2>, grid, dim3(DP_THREADS), 0, st, dd, S->L[li].wraw.p, S->xfrag.p, R[R_PART], ctr + li, total);
                break;
            default:
                hipLaunchKernelGGL(dense_pieces_kernel<3>, grid, dim3(DP_THREADS), 0, st, dd, S->L[li].wraw.p, S->xfrag.p, R[R_PART], ctr + li, total);
                break;
            }
            d.ksplit = dd.kparts;
        }
        const long long tot = (long long)d.N * d.OC;
        float* dst = li == 7 ? out : fc_out;
        float* pre = (li == 7 && tap == 10) ? tap_out : nullptr;
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)ew_blocks(tot)), dim3(EW_THREADS), 0, st, R[R_PART], S->L[li].bias.p, d.ksplit,
                           d.N, d.OC, li == 7 ? 2 : 1, dst, pre, live);
        mark(1);
        if (li == 5 && (rc = tapcopy(8, fc_out, A_FC6))) return rc;
        if (li == 6 && (rc = tapcopy(9, fc_out, A_FC7))) return rc;
        fc_in = fc_out;
        fc_out = (li == 5) ? R[R_FCB] : R[R_FCA];
    }
    if (cfg.profiling) {
        S->ev_valid = (evi == 14);
        if (S->ev_valid) ++S->ev_pass;
    }
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // namespace
#include "cnn_calibrate.hpp"
#include "cnn_range_policy.hpp"

namespace {

// host data -> a new device allocation in dst (owned by the state: released with it, also after a failure here)
template <typename T>
int upload(vpk_handle* h, DeviceBuffer<T>& dst, const T* src, size_t n) {
    VPK_HIP(h, hipMalloc(dst.out(), n * sizeof(T)));
    VPK_HIP(h, hipMemcpy(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return VPK_OK;
}
template <typename T>
int upload(vpk_handle* h, DeviceBuffer<T>& dst, const std::vector<T>& v) { return upload(h, dst, v.data(), v.size()); }

// every packed form of every layer's weights into the fresh state h->cnn, then the calibration.  Per layer: the dimension structs from
// cnn_model.hpp, the packers of the kernel headers, upload.  On failure the state is left as far as it got: vpk_cnn_load frees it.
int load_model(vpk_handle* h, const float* const blobs[16], const float* mean) {
    vpk_cnn_state* S = h->cnn;
    int rc;
    if ((rc = upload(h, S->mean, mean, IMAGE_PIXELS))) return rc;
    if (const char* e = getenv("VPK_CONV1_GROUP")) { const int v = atoi(e); if (v >= 1 && v <= 64) S->cfg.conv1_group = v; }
    if (const char* e = getenv("VPK_DENSE_PRESPLIT")) S->cfg.dense_presplit = atoi(e) != 0;
    for (int li = 0; li < 8; ++li) {
        const Topo& t = TOPO[li];
        const float* w = blobs[2 * li];
        Layer& l = S->L[li];
        const ConvDims& d = l.d = conv_dims(li);
        const size_t w_floats = (size_t)t.G * t.OC * d.K;
        const size_t p_floats = (size_t)t.G * d.Kp * d.Mp;
        {   // the forms the device packs from the raw weights (which live for this scope): the f32 GEMM's k-major panels ...
            DeviceBuffer<float> raw;
            VPK_HIP(h, hipMalloc(raw.out(), w_floats * sizeof(float)));
            VPK_HIP(h, hipMemcpy(raw.p, w, w_floats * sizeof(float), hipMemcpyHostToDevice));
            VPK_HIP(h, hipMalloc(l.wp.out(), p_floats * sizeof(float)));
            hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)ew_blocks((long long)p_floats)), dim3(EW_THREADS), 0, h->stream,
                               (const float*)raw.p, l.wp.p, t.G, t.OC, d.K, d.Kp, d.Mp);
            VPK_HIP(h, hipStreamSynchronize(h->stream));
            if (li == 5 || li == 6) {       // ... fc6, fc7: also as f32 in tile order for the pieces path (cnn_dense_pieces.hpp)
                const DenseDims& dd = l.dd = dense_dims(li);
                const long long total4 = (long long)dd.mtiles * dd.chunks * DP_BM * (DP_CHUNK / 4);
                VPK_HIP(h, hipMalloc(l.wraw.out(), (size_t)total4 * 16));
                hipLaunchKernelGGL(dense_tile_weights_kernel, dim3((unsigned)ew_blocks(total4)), dim3(EW_THREADS), 0, h->stream,
                                   (const float*)raw.p, l.wraw.p, t.OC, d.K, dd.chunks, total4);
                VPK_HIP(h, hipStreamSynchronize(h->stream));
                l.hscale = weight_scale_pow2(w, w_floats);
                // ... and as scaled fp16 pairs in the A-fragment order of dense_pairs_kernel (4 bytes per weight, like the f32 copy)
                const long long total16 = (long long)dd.mtiles * dd.chunks * 8 * 2 * 2 * 64;
                VPK_HIP(h, hipMalloc(l.wpair.out(), (size_t)total16 * 16));
                hipLaunchKernelGGL(dense_pair_weights_kernel, dim3((unsigned)ew_blocks(total16)), dim3(EW_THREADS), 0, h->stream,
                                   (const float*)raw.p, l.wpair.p, t.OC, d.K, dd.chunks, l.hscale, total16);
                VPK_HIP(h, hipStreamSynchronize(h->stream));
            }
        }
        if (li < 5 && (rc = upload(h, l.ktab, conv_ktab(li)))) return rc;
        if (li >= 1 && li <= 4) {   // conv2..5 in MFMA fragment order: three bf16 pieces of every weight (split GEMM and conv_pieces_kernel
                                    // read the same fragments), and scaled fp16 pairs: weights x 2^k (the largest in [2^13, 2^14))
            l.sd = split_dims(li);
            l.pd = piece_dims(li, false);
            l.pdh = piece_dims(li, true);
            std::vector<unsigned short> pk;
            pack_conv_fragments<3>(w, t.G, t.OC, t.IC, t.KH, l.sd.mblocks, 1.f, pk);
            if ((rc = upload(h, l.wsplit, pk))) return rc;
            l.hscale = weight_scale_pow2(w, w_floats);
            pack_conv_fragments<2>(w, t.G, t.OC, t.IC, t.KH, l.pdh.mblocks, l.hscale, pk);
            if ((rc = upload(h, l.whalf, pk))) return rc;
        }
        if (li == 0) {              // conv1 on the matrix cores: bf16 triples and scaled fp16 pairs in fragment order, bias - conv1(mean)
            std::vector<unsigned short> fr;
            conv1_pieces_weights(w, fr);
            if ((rc = upload(h, l.c1frag, fr))) return rc;
            l.c1scale = weight_scale_pow2(w, w_floats);
            conv1_pieces_weights(w, fr, 2, l.c1scale);
            if ((rc = upload(h, l.c1half, fr))) return rc;
            std::vector<float> cm;
            conv1_pieces_cmap(w, blobs[1], mean, cm);
            if ((rc = upload(h, l.c1map, cm))) return rc;
        }
        if (li >= 1 && li <= 4) {   // G g G^T of every filter, in the order the Winograd kernels stream it (cnn_winograd.hpp)
            std::vector<float> u;
            if (li == 1) {          // conv2: F(2 x 2, 5 x 5)
                winograd5_weights(w, t.G, t.OC, t.IC, u);
                l.wd5 = wino5_dims(li);
            } else {                // conv3..5: F(2 x 2, 3 x 3)
                winograd_weights(w, t.G, t.OC, t.IC, u);
                l.wd = wino_dims(li);
            }
            if ((rc = upload(h, l.wino, u))) return rc;
        }
        if ((rc = upload(h, l.bias, blobs[2 * li + 1], (size_t)t.G * t.OC))) return rc;
    }
    VPK_HIP(h, hipMalloc(S->range_word.out(), 256));
    VPK_HIP(h, hipMemset(S->range_word.p, 0, 256));
    VPK_HIP(h, hipMalloc(S->rc_list.out(), (1 + MAX_CHUNK) * sizeof(int)));
    VPK_HIP(h, hipMalloc(S->rc_total.out(), sizeof(unsigned long long)));
    VPK_HIP(h, hipMemset(S->rc_total.p, 0, sizeof(unsigned long long)));
    // the activation scales of the fp16-pair layers: six tapped forwards of the built-in calibration rasters on the f32 direct
    // kernels (calibrate()); their arena (batch 3) is released again so that the first real forward allocates once, for its batch
    rc = calibrate(h, nullptr, 0);
    S->act.reset();
    S->act_bytes = 0;
    S->act_batch = 0;
    return rc;
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
    h->cnn->cfg.profiling = on != 0;
    h->cnn->ev_valid = false;
    h->cnn->ev_pass = 0;
    return VPK_OK;
}

int vpk_cnn_set_fusion(vpk_handle* h, int on) {
    if (!h || !h->cnn) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_set_fusion before vpk_cnn_load");
    h->cnn->cfg.fusion = on < 0 ? 0 : (on > 4 ? 4 : on);
    return VPK_OK;
}

#ifdef W5_TIME
int vpk_dbg_w5(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(w5_dbg), sizeof(long long) * 256 * 12 * 8); }
int vpk_dbg_w3(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(w3_dbg), sizeof(long long) * 256 * 8 * 8); }
#endif

int vpk_cnn_set_algorithm(vpk_handle* h, int mode) {
    if (!h || !h->cnn) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_set_algorithm before vpk_cnn_load");
    if (mode < 0 || mode > 4) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_set_algorithm: mode must be 0 .. 4");
    h->cnn->cfg.algorithm = mode;
    return VPK_OK;
}

int vpk_cnn_set_precision(vpk_handle* h, int mode) {
    if (!h || !h->cnn) return vpk_fail(h, VPK_ERR_STATE, "vpk_cnn_set_precision before vpk_cnn_load");
    if (mode < 0 || mode > 3) return vpk_fail(h, VPK_ERR_ARG, "vpk_cnn_set_precision: mode must be 0 .. 3");
    cnn_config_set_precision(h->cnn->cfg, mode);       // 2, 3: force one tiling for every layer (development)
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
    const int rc = load_model(h, blobs, mean);
    if (rc != VPK_OK) vpk_cnn_free(h);          // the model stays unloaded: vpk_cnn_forward refuses (the message is the handle's)
    else h->cnn->loaded = true;
    return rc;
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
    vpk_cnn_state* S = h->cnn;
    if (policy) {
        int rc = vpk_reserve(h, S->img_range.out(), &S->img_range_bytes, (size_t)batch * sizeof(unsigned), "hipMalloc(per-image range flags)");
        if (rc) return rc;
        VPK_HIP(h, hipMemsetAsync(S->img_range.p, 0, (size_t)batch * sizeof(unsigned), h->stream));
        S->img_range_batch = batch;
    }
    // only the fp16-pair configuration can clamp: the recompute pass is not even launched for the others
    const bool recompute = policy && S->range_policy == 1 && S->cfg.precision == 0 && S->cfg.algorithm == 4;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        int nb = std::min(chunk, batch - b0);
        float* tp = (tap_out && tap >= 0 && tap <= 10) ? tap_out + (size_t)b0 * TAP_FLOATS[tap] : nullptr;
        const Images sp = sphere.at((size_t)b0);
        float* op = out + (size_t)b0 * OUTPUTS_PER_IMAGE;
        unsigned* img = policy ? S->img_range.p + b0 : nullptr;
        int rc = run_forward(h, S->cfg, sp, nb, op, tp ? tap : -1, tp, FwdCtl{S->range_word.p + (recompute ? 1 : 0), img, nullptr});
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
