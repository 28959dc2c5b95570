/*
 * vpk.h -- C-ABI of the MI355X-native vanishing-point hot path (libvpk.so).
 *
 * Drop-in boundary for the hot path of fkluger/vanishing_points_2017.  The reference is pure
 * Python and has no FFI of its own; its boundary for this path is the call surface of
 * evaluation.py (run_cnn :254, caffe_forward :34, run_em :295, run_em_single :332) plus
 * vp_localisation.expectation_maximisation (:168-172).  Each entry point below names the
 * reference interface it replaces (file:line under /root/reference).  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success or a negative vpk_status code; vpk_last_error()
 *     returns a human-readable message for the last failure on that handle.
 *   - unless a parameter is marked [host], buffers are DEVICE pointers (HBM-resident, e.g. a
 *     torch tensor's data_ptr()); all work is enqueued on the handle's HIP stream
 *     (vpk_set_stream) and is asynchronous with respect to the host unless stated.
 *   - one handle per process/GPU; a handle is thread-compatible (not thread-safe).
 *   - there is NO CPU fallback: on a machine without a gfx950 device vpk_create fails.
 */
#ifndef VPK_H_
#define VPK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPK_VERSION 110   /* 110 (round 6): + vpk_cnn_calibrate, vpk_cnn_get/set_activation_scales, vpk_cnn_range_flags, VPK_ERR_RANGE */

typedef struct vpk_handle vpk_handle;

enum vpk_status {
    VPK_OK = 0,
    VPK_ERR_ARG = -1,       /* bad argument (null pointer, size out of range)   */
    VPK_ERR_HIP = -2,       /* a HIP runtime call failed                        */
    VPK_ERR_NO_DEVICE = -3, /* no usable gfx950 device                          */
    VPK_ERR_STATE = -4,     /* call order (e.g. cnn_forward before cnn_load)    */
    VPK_ERR_LIMIT = -5,     /* problem exceeds a compiled-in limit (max VPs...) */
    VPK_ERR_RANGE = -6      /* the CNN's fp16-pair arithmetic left its calibrated value range (vpk_cnn_range_flags) */
};

/* per-image EM result status (status_out of vpk_em_batch) */
enum vpk_em_status {
    VPK_EM_OK = 0,            /* VPs returned                                                   */
    VPK_EM_NO_VP = 1,         /* reference returns the all-None result (vp_localisation.py:258-260,
                                 :402-404) -- also used where the reference would raise on an empty
                                 argmax (M == 0 at :349)                                         */
    VPK_EM_NO_INITIAL_VP = 2, /* reference raises ValueError from np.vstack([]) (:165)           */
    VPK_EM_NO_SLOT = 3        /* time-sliced launches only: no working-set slot became free within the launch's
                                 bounded wait (cannot happen while the documented slot invariant holds); the image
                                 was NOT refined and its other outputs are unset -- an error, never a result */
};
/* bit flags OR-ed into flags_out: situations where third-party tie-breaking is implementation
 * defined (Python heapq order inside sklearn's AgglomerativeClustering, vp_localisation.py:574) */
#define VPK_EM_FLAG_SPLIT_TIE 1u         /* exact tie between cluster distances during a split   */
#define VPK_EM_FLAG_SPLIT_DISCONNECTED 2u /* all-parallel line set: sklearn would complete graph */
#define VPK_EM_FLAG_VP_OVERFLOW 4u       /* more VPs than max_vp: result truncated               */

/* Mirrors the keyword defaults of expectation_maximisation (vp_localisation.py:168-172). */
typedef struct vpk_em_params {
    int32_t num_iter;          /* 100   */
    int32_t do_merge;          /* 1     */
    int32_t do_split;          /* 1     */
    int32_t do_iterations;     /* 1     */
    int32_t use_weights;       /* 1     */
    int32_t num_init_vp;       /* 25    */
    int32_t split_merge_freq;  /* 10    */
    int32_t num_min_lines;     /* 3     */
    double wbias;              /* 1.0   */
    double merge_thresh;       /* 1e-3  */
    double outlier_thresh;     /* 1.96^2 */
    double final_convergence;  /* 5e-3  */
    double s_thresh;           /* 1e-200 */
} vpk_em_params;

/* ---- lifetime ------------------------------------------------------------------------------ */
/* replaces: caffe.set_mode_gpu(); caffe.set_device(gpu_id)  (evaluation.py:20-21) */
int vpk_create(int device, vpk_handle** out);
int vpk_destroy(vpk_handle* h);
/* use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int vpk_set_stream(vpk_handle* h, void* hip_stream);
/* the hipStream_t the handle enqueues on */
void* vpk_get_stream(const vpk_handle* h);
int vpk_synchronize(vpk_handle* h);
const char* vpk_last_error(const vpk_handle* h);
int vpk_version(void);
void vpk_em_default_params(vpk_em_params* p);
/* device properties as seen by the library: [0]=CU count, [1]=LDS bytes per block, [2]=gfx arch number */
int vpk_device_info(const vpk_handle* h, int32_t info[4]);
/* Upper bound on the persistent workgroups (= CUs held) of one vpk_em_batch launch; 0 = one per image up
 * to the CU count (lowest latency for a single call).  A pipeline that runs other kernels beside the EM
 * (the reference's run_cnn of the next batch, evaluation.py:254-292) sets about batch/3: the images
 * queue inside the launch, which then lasts about as long as its slowest image anyway and leaves the
 * other CUs to the CNN. */
int vpk_em_set_workgroups(vpk_handle* h, int max_workgroups);
/* Which kernel evaluates weight_matrix (vp_localisation.py:515-524) inside the EM.  0 (default): the row-sliced kernel
 * (partial sums never leave the wave, operands by DPP row broadcast) wherever its LDS panel fits, the round-1/2 kernels
 * elsewhere; 1: always the round-1/2 kernels; 2: for images of up to 448 lines the sparse kernel (the terms whose operand
 * p_vl * lweight is exactly zero -- more than four in five -- are left out; a wave per group of VPs, lsim staged through
 * LDS by DMA once per call; measured slower than the dense kernel, kept as an option).  All of them sum every (column,
 * VP) in the same order, so every output of vpk_em_batch / vpk_weight_matrix is bit-identical under the three settings
 * (tests/test_gpu_em.py): the switch exists for that test and for A/B timing.  Mode 1 also selects the earlier forms of the
 * other phases that have been rebuilt with the same arithmetic since (round 6: the E-step's one thread per line, the serial
 * VP compaction, the row-by-row pair pass of calc_lsim for images of 512 lines and more, the M-step's four loads in flight
 * there; vpk_pairwise honours it too) -- the same test therefore pins those rebuilds bit for bit.  Likewise the E-step's line
 * part: with the operand panel in LDS the default evaluates the exp and the division to p_vl only for the terms that do not
 * underflow, mode 1 for every (line, VP) pair (tests/test_gpu_em_estep_zeros.py). */
int vpk_em_set_smoother(vpk_handle* h, int mode);
/* LDS the EM workgroup may plan with for its weight_matrix operand panel and the split's cluster matrix, in doubles;
 * 0 (default) = everything a CU has beside the workgroup's state (~18 800).  A smaller budget sends images down the
 * paths that larger images take by necessity -- the chunked smoother (operands staged through LDS piece by piece), the
 * split's distance matrix and direction vectors in HBM.  Results agree to rounding, not to the bit: the chunked
 * smoother sums a column's rows in ONE chain where the in-LDS kernels sum eight row slices; the parity bar
 * (assignments exact, VPs 1e-4) holds either way, and the GPU tests use the switch to run those paths on the
 * reference's small goldens.  Applies to vpk_em_batch and vpk_weight_matrix. */
int vpk_em_set_lds_panel(vpk_handle* h, int doubles);
/* distance_measure of expectation_maximisation (vp_localisation.py:170, :196-203) for every vpk_em_batch launch on this
 * handle: VPK_DIST_ANGLE (default) or VPK_DIST_DOTPROD (enum vpk_dist_measure below), each its own instantiation of the
 * persistent kernel.  Under "dotprod" the E-step's distance is (l . v)^2 on the normalised line and the VP as given, the
 * outlier test of calc_vp_line_counts compares |l . v| (:496), and the variance starts from and is capped at 1e-3 times
 * the prior's sigma and 1e-3 (:199-201) instead of 1e-6.  VPK_DIST_AREA and any other value: VPK_ERR_ARG (the reference
 * asserts at :203).  VPK_ERR_STATE while time-sliced launches have images parked (a parked image is resumed by the
 * measure that parked it): vpk_em_flush first.  The fine-grained entry points (vpk_estep, vpk_line_counts, ...) and
 * the VP-set batch calls stay "angle". */
int vpk_em_set_distance_measure(vpk_handle* h, int measure);

/* Time-sliced EM launches for pipelines (run_cnn of batch k+1 while the EM of batch k is unfinished,
 * evaluation.py:254-329).  The EM of a never-converging image takes 99 iterations (vp_localisation.py:256)
 * where the average image takes ~25, so a launch that runs every image to completion holds its CUs for the
 * slowest one.  With slice_ms > 0 every vpk_em_batch launch on this handle gets a time budget instead: an
 * image still iterating when it expires is suspended at the top of its next iteration (its state is parked in
 * HBM) and resumed -- by any workgroup, before fresh images -- in the next launch on the handle; images that
 * had not started yet are parked likewise.  Results are bit-identical to an uninterrupted run.  Consequences
 * for the caller: the outputs of a call are complete only after vpk_em_flush (or once later launches have
 * finished its images), and the INPUT buffers of a call (l, lp, cnn, sphere, init_vp) as well as its output
 * buffers must stay alive and untouched until then.  n_max: slots are sized for images of up to n_max lines
 * (a later batch with more lines, or with other EM parameters, needs a vpk_em_flush first).
 * slice_ms = 0 switches back (flushing first).  replaces: nothing in the reference (its run_em is one
 * sequential loop, evaluation.py:309-329); this is what lets CNN and EM share one GPU without a tail. */
int vpk_em_set_time_slice(vpk_handle* h, double slice_ms, int n_max);
/* enqueue one launch that runs every parked image to completion (asynchronous on the handle's stream) */
int vpk_em_flush(vpk_handle* h);

/* ---- CNN (AlexNet-500, cnn/deploy.prototxt:1-304) -------------------------------------------- */
/* replaces: caffe.Net(model_def, model_weights, caffe.TEST) + read_mean_blob
 * (evaluation.py:17-31).  blobs [host]: 16 host pointers to fp32 arrays in Caffe layout,
 * order conv1.w, conv1.b, conv2.w, conv2.b, ..., conv5.b, fc6.w, fc6.b, fc7.w, fc7.b, fc8.w,
 * fc8.b (OIHW / (out,in)); mean [host]: 500*500 fp32 (mean.binaryproto, 1x1x500x500).
 * Copies to HBM (synchronous), packs the weights for every arithmetic mode, and CALIBRATES the default mode's activation
 * scales: six forwards of three built-in rasters (batch 3) on the f32 direct kernels, tapped at the inputs of conv2..5, fc6 and
 * fc7 -- ~20 ms of GPU time; see vpk_cnn_calibrate.  The response maps of the default mode depend on those scales (to rounding,
 * not beyond: tests/test_gpu_cnn.py), which are a function of the weights and the mean alone -- two loads of one model give
 * the same bits.  If calibration fails the model stays unloaded. */
int vpk_cnn_load(vpk_handle* h, const float* const blobs[16], const float* mean);
/* The value range of the default arithmetic (vpk_cnn_set_algorithm(4): scaled fp16 pairs) and how it is kept.
 * A layer's input x reaches the matrix cores as the fp16 pair of s x, s a power of two per consuming layer (conv2..5, fc6, fc7).
 * s is chosen so that the LARGEST |x| of that blob over a calibration set lands in [32, 64): rasters whose activations are up to
 * 2^10 x those of the calibration set stay finite, and smaller values keep full precision (22 bits) down to 2^-13 of the
 * calibration maximum and an absolute error below 2^-31 of it beyond that.  The built-in set is a sparse raster, a raster of
 * 1000 blended strokes (the density of a 1000-line sphere image, evaluation.py:12-14) and the all-255 raster.
 *   vpk_cnn_calibrate      rasters: n x 500 x 500 uint8 (DEVICE, 4-byte aligned) of the caller's choice -- the scales are set
 *                          from THESE rasters' blob maxima alone; n = 0 (rasters ignored): the built-in set again.  Runs
 *                          6 x ceil(n / 8) forwards on the f32 direct kernels and waits for them.
 *   vpk_cnn_get/set_activation_scales   the six powers of two (inputs of conv2, conv3, conv4, conv5, fc6, fc7); set: each
 *                          must be a power of two (VPK_ERR_ARG otherwise).  Restoring a saved vector restores the bits.
 *   vpk_cnn_range_flags    fp16's largest finite number is 65 504.  Every kernel that writes a scaled pair clamps to it and ORs
 *                          bit li (1 = conv2 ... 4 = conv5, 5 = fc6, 6 = fc7: the CONSUMING layer) into a device word when a value
 *                          reached it; nothing non-finite is ever produced by the scaling.  This call waits for the handle's
 *                          stream, returns the word in *flags_out (may be NULL), clears it, and returns VPK_ERR_RANGE when it
 *                          was non-zero (vpk_last_error names the layers), VPK_OK otherwise: it covers every forward on the
 *                          handle since the previous call.  A flagged response map was computed from clamped activations -- it
 *                          is finite but NOT the net's: recalibrate, or switch to vpk_cnn_set_algorithm(2) (exact operands, no
 *                          range to leave).  The reference's f32 Caffe forward (evaluation.py:34-38) has no such limit; this
 *                          is how the limit of the faster arithmetic is made impossible to miss. */
int vpk_cnn_calibrate(vpk_handle* h, const uint8_t* rasters, int n);
int vpk_cnn_get_activation_scales(vpk_handle* h, float scales[6]);
int vpk_cnn_set_activation_scales(vpk_handle* h, const float scales[6]);
int vpk_cnn_range_flags(vpk_handle* h, uint32_t* flags_out);
/* Per-image flags and the exact recompute of flagged images (the range POLICY of the handle).
 *   vpk_cnn_set_range_policy   0 = RAISE (the default): the above, nothing else changes.  1 = RECOMPUTE_EXACT: after the pair
 *                          forward of each chunk, the images whose pair forward clamped anything are found on the device and
 *                          recomputed there with exact operands (the vpk_cnn_set_algorithm(2) forward with the default conv1, the
 *                          same bits as that forward run on those rasters alone as one batch in their order); their maps replace the
 *                          pair results in `out` on the handle's stream, before anything behind the forward reads them, with no
 *                          host wait.  A recomputed image is NOT reported through vpk_cnn_range_flags -- its map is the net's --
 *                          so that call returns VPK_OK for it.  Any other value: VPK_ERR_ARG.  Modes other than the default
 *                          arithmetic (vpk_cnn_set_algorithm(0 .. 3), vpk_cnn_set_precision(1)) never clamp and run no pass.
 *   vpk_cnn_image_range_flags  waits for the stream and copies the per-image bits (as in vpk_cnn_range_flags) of the LAST
 *                          vpk_cnn_forward (a vpk_pipeline_step's included) into flags_out[0 .. batch); `batch` must equal that
 *                          call's (VPK_ERR_ARG otherwise).  Under both policies; under RECOMPUTE_EXACT they name the images that
 *                          were recomputed.  vpk_cnn_forward_tap (debugging) ignores the policy and keeps no per-image bits.
 *   vpk_cnn_recomputed     waits for the stream, returns in *n_out how many images were recomputed since the previous call
 *                          and clears the count. */
int vpk_cnn_set_range_policy(vpk_handle* h, int policy);
int vpk_cnn_image_range_flags(vpk_handle* h, int batch, uint32_t* flags_out);
int vpk_cnn_recomputed(vpk_handle* h, int64_t* n_out);
/* replaces: caffe_forward (evaluation.py:34-38) for a batch: sphere B x 500 x 500 uint8 ->
 * out B x 20 x 20 fp32 (sigout).  max batch per call is unbounded (internally chunked).  `sphere` must be 4-byte
 * aligned (device allocations are). */
int vpk_cnn_forward(vpk_handle* h, const uint8_t* sphere, int batch, float* out);
/* debugging/parity: run the net and also return an intermediate blob by name index
 * (0=conv1 relu, 1=pool1, 2=conv2, 3=pool2, 4=conv3, 5=conv4, 6=conv5, 7=pool5, 8=fc6, 9=fc7,
 * 10=fc8 pre-sigmoid); tap_out must hold batch * blob_size fp32. */
int vpk_cnn_forward_tap(vpk_handle* h, const uint8_t* sphere, int batch, float* out, int tap,
                        float* tap_out);
/* replaces: caffe_forward (evaluation.py:34-38) for float images: image B x 500 x 500 fp32 (DEVICE, 16-byte aligned), the
 * values Caffe's float32 data blob holds BEFORE the mean is subtracted (any real value; a raster in [0, 1], a blurred or resampled
 * one) -> out B x 20 x 20 fp32 (sigout).  Everything else is vpk_cnn_forward's / vpk_cnn_forward_tap's: unbounded batch
 * (internally chunked), asynchronous on the handle's stream, the same range word, per-image bits (vpk_cnn_image_range_flags
 * names the last forward of either type) and range policy.  Every arithmetic mode accepts it except vpk_cnn_set_fusion(4)
 * (VPK_ERR_STATE: its fp16 conv1 needs integer pixels).  The default conv1 splits each pixel into three exact bf16 pieces
 * (six products per weight and pixel instead of three); an integer-valued image in 0 .. 255 gives the same bits as its uint8
 * raster.  Non-finite pixels are the caller's business, as in Caffe: nothing checks for them.  The activation scales stay
 * those of uint8 calibration (vpk_cnn_calibrate): images far beyond the calibration set's magnitude are caught by the range
 * flags and the range policy above, as for rasters. */
int vpk_cnn_forward_f32(vpk_handle* h, const float* image, int batch, float* out);
int vpk_cnn_forward_tap_f32(vpk_handle* h, const float* image, int batch, float* out, int tap, float* tap_out);

/* How the net's layers are computed.  The reference runs Caffe in fp32 (deploy.prototxt, evaluation.py:20: cuDNN's pick of
 * algorithm per layer); every setting below keeps f32 operands, f32 accumulation and f32 results -- what changes is which matrix
 * instruction multiplies, in how many pieces the operands reach it, and where the sums are rounded.  Each setting's error against the SAME net evaluated in float64 is
 * measured by tests/test_gpu_cnn.py and tests/test_gpu_cnn_modes.py; the defaults are, at every tap, no further from it than the
 * f32-input direct kernels.
 *
 * conv1 + relu1 + norm1 + pool1 (deploy.prototxt:9-55):
 *   3 (default)  ONE kernel on the bf16 matrix cores with EXACT operands: the uint8 raster is one bf16 piece, each weight the sum
 *                of three, `- mean` (evaluation.py:35) a constant map made in float64 at load -- three bf16 products per f32
 *                product, none of them rounded (csrc/cnn_conv1_pieces.hpp).  The 96 x 123 x 123 conv1 blob is never written.
 *   4            the same kernel with the weights as scaled fp16 PAIRS (two products: the raster's integers are exact fp16 numbers too);
 *                no faster -- the kernel is bound by its LDS epilogue, not by the matrix pipe (0.366 against 0.375 ms) -- and not the default
 *                (22 of the weights' 24 bits: at pool1 it meets the factor-1 rule against mode 1 -- 2.4e-7 against 5.9e-7 of the blob's
 *                scale --, and so does the output under vpk_cnn_set_algorithm(4); the output under algorithm 0 is NOT held to
 *                factor 1, only to 2e-5: the f32 chains behind it dominate, measured 1.03 x mode 1's; tests/test_gpu_cnn_modes.py)
 *   1            ONE kernel on the f32-input matrix instructions (v_mfma_f32_16x16x4_f32: an f32 FMA chain over the 121 taps)
 *   2            the implicit-GEMM kernel with the fused LRN / pooling epilogue
 *   0            separate conv1 and LRN / pooling kernels (also used whenever tap 0 is requested) */
int vpk_cnn_set_fusion(vpk_handle* h, int mode);
/* Arithmetic of conv2..conv5 (deploy.prototxt:56-174) when vpk_cnn_set_algorithm is 0:
 *   0 (default)  f32-input matrix instructions (v_mfma_f32_32x32x2_f32): bit-for-bit an f32 FMA chain per output
 *   1            every f32 operand as the exact sum of three bf16 pieces, six bf16 matrix products per f32 product
 *                (everything above 2^-24 of the product), f32 accumulation, implicit GEMM (csrc/cnn_split_gemm.hpp); per layer
 *                the faster of its two tilings (conv2 / conv3: two 4-wave workgroups per CU, conv5: one 8-wave workgroup)
 *   2, 3         (development) as 1, but force one tiling of the split GEMM for every layer: 2 = one 8-wave workgroup per CU,
 *                3 = two 4-wave workgroups per CU (conv4 has one tiling only).  The same arithmetic as 1.
 * Any other value: VPK_ERR_ARG. */
int vpk_cnn_set_precision(vpk_handle* h, int mode);
/* Algorithm of conv2..conv5 and fc6 (precision 0):
 *   4  (default) DIRECT convolutions (and fc6's weight stream) on the fp16 matrix cores, every f32 operand as a SCALED PAIR of fp16
 *      numbers h0 = fp16(s x), h1 = fp16(s x - h0) -- 22 of its 24 significand bits, the remainder below 2^-23 |x| -- and THREE exact
 *      products per f32 product (h0 h0', h0 h1', h1 h0'; the fourth, h1 h1', is at most 2^-22 and typically 2^-24 of the product).  s is a power of two: per layer
 *      for the weights (the largest lands in [2^13, 2^14)), per consuming layer for the activations (calibrated at load: vpk_cnn_calibrate
 *      above, with the range check that goes with it); the epilogue multiplies by the exact reciprocal.
 *      Sums as in 2: the products of a kernel row x 16 channels (all taps of a 3 x 3 layer) accumulate from zero and join the f32
 *      accumulator with ONE rounding.  Half the matrix instructions of 2 -- which matters because the matrix cores are
 *      power-limited with real operands (1.7 PFLOP/s sustained against the 2.5 dense peak, scripts/ubench/mfma_f16_pairs.hip).
 *      Error against the float64 net (B = 3, scale of each blob): conv2 0.25e-6, conv3..5 0.4-0.5e-6, fc6 0.4e-6 -- at every tap
 *      below 2's and 2-4 x below the f32 direct kernels' (csrc/cnn_conv_pieces.hpp, csrc/cnn_dense_pieces.hpp)
 *   2  conv2 (5 x 5, 2 x 48 -> 128 channels) and fc6 on the bf16 matrix cores with EXACT operands -- three bf16 pieces per operand,
 *      six products per f32 product, block sums as in 4 (error 0.2e-6; the f32 direct kernel's is 1.0e-6) --; conv3..conv5 as in 1
 *   1  Winograd's minimal filtering on the f32-input matrix instructions: conv2 by F(2 x 2, 5 x 5) (36 instead of 100 products per
 *      2 x 2 outputs and input channel), conv3..conv5 by F(2 x 2, 3 x 3) (16 instead of 36); input / output transforms in f32.
 *      Same arithmetic type and accumulation width as the direct form; the rounding differs (products of transformed
 *      operands, shorter sums): error 0.6-0.8e-6 against 1.0-2.0e-6 for the direct kernels (csrc/cnn_winograd.hpp)
 *   0  direct: implicit GEMM over the taps -- every output is one f32 FMA chain over (channel, tap)
 *   3  (measurements) conv2, conv3 and conv5 as in 2's conv2, conv4 as in 1 */
int vpk_cnn_set_algorithm(vpk_handle* h, int mode);

/* per-layer device time of the last vpk_cnn_forward (single chunk), from HIP events recorded on
 * the handle's stream between the layers: ms[13] = conv1, norm1, pool1, conv2, norm2, pool2, conv3,
 * conv4, conv5, pool5, fc6, fc7, fc8 (with the fused first stage: conv1 = the whole fused kernel, norm1 = pool1 = 0).
 * vpk_cnn_last_layer_ms waits for the pass to finish. */
int vpk_cnn_set_profiling(vpk_handle* h, int on);
int vpk_cnn_last_layer_ms(vpk_handle* h, float ms[13]);
/* the same, averaged over the profiled passes since the last vpk_cnn_set_profiling call (at most the last 64); *passes
 * (may be NULL) = how many.  Waits for them to finish. */
int vpk_cnn_mean_layer_ms(vpk_handle* h, float ms[13], int* passes);

/* ---- sphere rasteriser (sphere_mapping.py:36-72) ----------------------------------------------- */
/* replaces: get_sphere_image / sphere_line_plot (evaluation.py:12-14).  l: sum(N) x 3 fp64
 * homogeneous lines, offsets [host]: B+1 int64 prefix of line counts; out: B x size x size uint8,
 * image row 0 = beta = +pi/2.  alpha = per-line blend weight (0.1 in the reference).  size 8..1024.
 * The reference's matplotlib / Agg pipeline stage by stage (10 000 samples per line, PathSimplifier, 1 pt stroke,
 * anti-aliased scanline coverage, plain 8-bit "over" in line order, black axes spines last): pixel-exact.
 * Asynchronous on the handle's stream, except that `offsets` (caller-owned host memory) is uploaded and waited for when
 * it differs from the previous call's on this handle -- a pipeline that rasterises the same batch structure again does
 * not wait for anything.  An image without lines gets the frame-only canvas, like the reference's; when the whole
 * batch has no line, l may be NULL.  Workspace (kept on the handle, grown on demand), per line of the largest chunk of
 * <= 49 152 lines: ~38 KB of outline scratch + 64 x size bytes of row table + 16 KB of coverage pool (~86 KB per line at
 * size 500: 4.2 GB for a full chunk; the pool is never smaller than 8 x size x (size + 2) bytes and must stay below
 * 4 GiB).  An image is never split over chunks, so that bound limits the lines of ONE image: (N + 4) x 16 KB < 4 GiB, i.e.
 * at most 262 139 lines; in `alternative` mode (below) the pool is size x (size + 2) bytes per line and chunks hold at most
 * min(49 152, 3 GiB / (size x (size + 2))) lines, so an image has at most floor((2^32 - 1) / (size x (size + 2))) - 4
 * lines (17 107 at size 500, 4 084 at size 1024).  One line more: VPK_ERR_LIMIT before anything is allocated or launched,
 * the message names the largest count.
 * VPK_ERR_ARG, likewise before anything is done: a null handle / offsets / out, batch < 1, size outside 8..1024, alpha
 * outside 0..1 (NaN included), offsets that decrease, l == NULL although the batch has lines. */
int vpk_sphere_raster(vpk_handle* h, const double* l, const int64_t* offsets, int batch, int size,
                      double alpha, uint8_t* out);
/* replaces: the `alternative` keyword of sphere_line_plot (sphere_mapping.py:58-59; no caller in the reference passes it):
 * on != 0 makes the following vpk_sphere_raster calls on this handle draw beta = atan(-c / (a cos alpha + b sin alpha))
 * instead of atan((-a sin alpha - c cos alpha) / b). */
int vpk_sphere_raster_set_alternative(vpk_handle* h, int on);
/* per-image flags of the LAST vpk_sphere_raster call on this handle (waits for it): bit 0 = a line produced more outline
 * vertices / coverage than the kernel's buffers hold and was truncated or dropped (never seen on real line sets: a
 * simplified curve keeps 30-100 of its 10 000 samples).  `batch` must be that call's batch (VPK_ERR_ARG otherwise). */
int vpk_sphere_raster_flags(vpk_handle* h, int batch, uint32_t* flags_out);

/* ---- front end: line segment detection (vpk_lsd_detect: HOST code, host pointers) -------------------------------- */
/* replaces: lsdpython.lsd.detect_line_segments(image) as called by detect_lsd_lines (evaluation.py:227-251; the
 * detector itself is an un-vendored submodule of the reference, .gitmodules:1-3 -- parity unpinned, see
 * csrc/lsd_device.hpp, the detector's one source; csrc/lsd_host.hpp runs it for one image).  A null image or n_out,
 * width or height < 8, max_segments < 0, rows without a buffer, a scale that is not > 0: VPK_ERR_ARG.  image [host]: height x width fp64 grey levels 0..255, row-major; scale: Gaussian sub-sampling
 * factor (0.8 = LSD's default).  out [host]: up to max_segments rows of 7 doubles (x1, y1, x2, y2, width, p,
 * -log10(NFA)) in pixel coordinates of the input image; *n_out = number of segments found (if it exceeds
 * max_segments only the first max_segments were written: call again with a larger buffer).  No GPU involved. */
int vpk_lsd_detect(const double* image, int width, int height, double scale, double* out, int max_segments, int* n_out);
/* The same detector, compiled from the same source, for a batch of images on the GPU (csrc/vpk_lsd_gpu.hip; the rules,
 * the workspace layout and the chunks below: csrc/lsd_plan.hpp).  Per image exactly what vpk_lsd_detect does: the same
 * rows in the same order, the same argument rules (width, height >= 8 and scale > 0, else VPK_ERR_ARG)
 * and the same overflow rule; coordinates and -log10(NFA) may differ from the host's in the last bits only, where the
 * device's atan2 / sin / cos / exp / log differ from the host libm's.  Everything else -- the
 * grid-wide passes, the seed order, the wave-split region stage, the chunking -- is pinned bit for bit: under the
 * portable math policy (vpk_lsd_set_math) the rows equal the host's under that policy byte for byte
 * (tests/test_gpu_lsd_exact.py), and both equal recorded rows (tests/golden/lsd/lsd_portable.npz).
 *   dims         [host] B x 2 int32: width, height of each image
 *   pix_offsets  [host] B+1 int64 prefix sums of width * height (offsets of the images in `images`)
 *   images       concatenated row-major fp64 grey levels 0..255
 *   out          B x max_segments x 7 fp64: image b's rows start at b * max_segments
 *   n_out        B int32: image b's segment count (may exceed max_segments: only the first max_segments rows are written)
 * Asynchronous on the handle's stream; batch = 0 does nothing.  The workspace is kept on the handle and grows on demand;
 * a batch whose workspace would pass the handle's limit runs in chunks inside the call.  Rows do not depend on the rest
 * of the batch or on the chunking.  An image with a side beyond 2^20 pixels or more than 2^30 sub-sampled pixels:
 * VPK_ERR_LIMIT. */
int vpk_lsd_detect_batch(vpk_handle* h, int batch, const int32_t* dims, const int64_t* pix_offsets, const double* images,
                         double scale, double* out, int max_segments, int32_t* n_out);
/* Workspace limit of vpk_lsd_detect_batch in bytes (0 = the default, 4 GiB; about 43 bytes per sub-sampled pixel, so
 * 8.5 MB for a 640 x 480 image at scale 0.8).  An image larger than the limit runs alone. */
int vpk_lsd_set_workspace_limit(vpk_handle* h, size_t bytes);
/* TEST HOOK: the elementary functions vpk_lsd_detect_batch's gradient and region kernels call on this handle.
 * mode 0 (default) = the device libm, the product's; 1 = the portable functions of csrc/lsd_portable_math.hpp, which
 * give the host build's bits on the device, so the batch's rows can be compared with the host build byte for byte.
 * Any other mode: VPK_ERR_ARG.  Not used by any product path. */
int vpk_lsd_set_math(vpk_handle* h, int mode);

/* ---- front end: decoded images -> grey levels, detector rows -> lines (csrc/vpk_frontend.hip) --------------------- */
/* replaces: the host half of the reference's front end around the detector for a batch of decoded images --
 * `convert -resize SxS` (evaluation.py:141-143; this package's stand-in is Pillow's Image.resize(LANCZOS),
 * frontend.resize_to_fit) and rgb2gray (evaluation.py:148-150) -- with the grey levels detect_lsd_lines hands to the
 * detector (evaluation.py:227-236).  Per image: a separable Lanczos fit-resize in Pillow's fixed-point arithmetic (weights
 * made on the host with the C library's sin, integer passes on the device, the horizontal pass first and clipped to uint8; a
 * pass whose size is unchanged is skipped) -- byte for byte Pillow's uint8 result -- then
 *   grey = (((r / 255) * 0.2125 + (g / 255) * 0.7154) + (b / 255) * 0.0721) * 255   (3 channels, left to right, no FMA)
 *   grey = (g / 255) * 255                                                          (1 channel)
 * (frontend.rgb2gray rounds the same sum in the order of its BLAS dot: a few ulp apart; csrc/image_device.hpp).
 *   dims         [host] B x 5 int32: in_w, in_h, channels (1 or 3), out_w, out_h
 *   in_offsets   [host] B+1 int64 prefix sums of in_w * in_h * channels (byte offsets of the images in `images`)
 *   images       concatenated row-major interleaved uint8 pixels
 *   out_offsets  [host] B+1 int64 prefix sums of out_w * out_h (pixel offsets of the images in `grey_out`)
 *   resized_out  NULL or the resized uint8 images, one after the other (image b at the sum of out_w * out_h * channels
 *                of the images before it)
 *   grey_out     fp64 grey levels 0..255: exactly the `images` / `pix_offsets` vpk_lsd_detect_batch takes, with dims
 *                (out_w, out_h)
 * Channels other than 1 or 3, a side < 1 or offsets that disagree with dims: VPK_ERR_ARG; a side beyond 2^20:
 * VPK_ERR_LIMIT.  Asynchronous on the handle's stream; batch = 0 does nothing. */
int vpk_image_prepare_batch(vpk_handle* h, int batch, const int32_t* dims, const int64_t* in_offsets, const uint8_t* images,
                            const int64_t* out_offsets, uint8_t* resized_out, double* grey_out);
/* replaces: the arithmetic after the detector in detect_lsd_lines (evaluation.py:237-251: centre, divide by half of the
 * long side, y up) and the homogeneous lines of create_data_pickles (evaluation.py:161-168: np.cross((x1, y1, 1),
 * (x2, y2, 1))) -- the same fp64 operations, each rounded on its own, so the results equal numpy's byte for byte.
 *   dims          [host] B x 2 int32: width, height of the image each detector row belongs to (vpk_lsd_detect_batch's dims)
 *   rows          B x max_segments x 7 fp64: vpk_lsd_detect_batch's `out`
 *   line_offsets  [host] B+1 int64 prefix sums of the images' segment counts (vpk_lsd_detect_batch's n_out); a count
 *                 above max_segments: VPK_ERR_ARG -- those rows were not written: detect again with a larger buffer
 *   lp_out        sum(N) x 4 fp64 (x1, y1, x2, y2) normalised segments, vpk_em_batch's `lp`
 *   l_out         sum(N) x 3 fp64 homogeneous lines, vpk_sphere_raster's / vpk_em_batch's `l`
 *   nfa_out       sum(N) fp64 -log10(NFA)
 * Each output may be NULL (not written).  Asynchronous on the handle's stream; batch = 0 does nothing. */
int vpk_lsd_rows_to_lines(vpk_handle* h, int batch, const int32_t* dims, const double* rows, int max_segments,
                          const int64_t* line_offsets, double* lp_out, double* l_out, double* nfa_out);

/* ---- EM refinement (vp_localisation.py:168-450) ------------------------------------------------ */
/* replaces: run_em / run_em_single -> expectation_maximisation (evaluation.py:295-354) for a
 * batch of images.  One workgroup runs the whole EM of one image; images are independent.
 *   offsets  [host] B+1 int64 prefix sums of per-image line counts N_b
 *   l        sum(N) x 3 fp64, normalised IN PLACE (reference :185-186,:226)
 *   lp       sum(N) x 4 fp64 segment end points (x1,y1,x2,y2)
 *   cnn      B x 400 fp32 (20x20 sigout, row = beta bin)
 *   sphere   B x size x size uint8
 *   init_vp  NULL or B x n_init x 3 fp64 (reference keyword init_vp)
 *   max_vp   row capacity of the per-image outputs below
 * outputs (device): vp_out B x max_vp x 3, sigma_out / counts_out / counts_w_out B x max_vp,
 *   num_vp_out B, assoc_out sum(N) int64 (-1 = outlier), iterations_out B, status_out B
 *   (vpk_em_status), flags_out B (VPK_EM_FLAG_*), metric_out NULL or sum(N) x max_vp fp64
 *   (decision_metric, [line][vp]), trace_out NULL or B x (num_iter+1) x 12 fp64
 *   (row i: M after the M-step, max_err, M at the end of the iteration, event bits, then device
 *   microseconds spent in E-step / smoothing / M-step / whole iteration; row num_iter: microseconds
 *   of pairwise setup, remaining setup, whole image, M after the final merge / hard M-step / winner
 *   selection, then microseconds inside the single-pass smoother: staging + reduction, main loop). */
int vpk_em_batch(vpk_handle* h, int batch, const int64_t* offsets, double* l, const double* lp,
                 const float* cnn, const uint8_t* sphere, int sphere_size, const double* init_vp,
                 int n_init, const vpk_em_params* p, int max_vp, double* vp_out, double* sigma_out,
                 double* counts_out, double* counts_w_out, int32_t* num_vp_out, int64_t* assoc_out,
                 int32_t* iterations_out, int32_t* status_out, uint32_t* flags_out,
                 double* metric_out, double* trace_out);
/* EM_result['distribution'] (vp_localisation.py:441: the probability_functions.PDF of the LAST calc_probabilities call,
 * probability_functions.py:99-120) of every image of the NEXT vpk_em_batch call (the setting is consumed by that call; a
 * NULL argument clears it).  Device buffers, rows beyond an image's VP count are zero:
 *   p_v B x max_vp (PDF.v), angles B x max_vp x 2 (PDF.angles: alpha, beta), p_l sum(N) (PDF.l),
 *   p_lv sum(N) x max_vp (PDF.lv, [line][vp]), p_vl sum(N) x max_vp (PDF.vl transposed to [line][vp]),
 *   lvsq sum(N) x max_vp (PDF.lvsq).  Not available together with time-sliced launches. */
typedef struct vpk_em_dist_out {
    double* p_v;
    double* angles;
    double* p_l;
    double* p_lv;
    double* p_vl;
    double* lvsq;
} vpk_em_dist_out;
int vpk_em_set_distribution_out(vpk_handle* h, const vpk_em_dist_out* d);
/* bytes of device workspace the next vpk_em_batch with these sizes will hold (informational) */
size_t vpk_em_workspace_bytes(const vpk_handle* h, int batch, int n_max, const vpk_em_params* p,
                              int n_init);

/* ---- one pipeline step as one host call ------------------------------------------------------- */
/* replaces: one batch's worth of run_cnn followed by run_em (evaluation.py:254-329) in a pipeline that overlaps
 * consecutive batches: the CNN forward on `cnn`'s stream, then -- ordered behind it by an event, without a host wait
 * -- a copy of the resident lines into l_work, the EM on `em`'s stream with the CNN's response maps as its prior, and
 * optionally the fixed-size result records a multi-GPU run gathers (layout of vpk_build_records).  Everything is
 * enqueued from C++: the host spends tens of microseconds per step.  Buffers as for vpk_cnn_forward / vpk_em_batch;
 * `events`: NULL or four hipEvent_t of the caller (any may be NULL) recorded before / after the CNN on its stream and
 * before / after the EM on its stream.  `cnn` and `em` may be the same handle (one stream: the stages run in turn).
 * The buffers of a step must not be reused before its EM has finished: `reuse_event` expresses that on the device.
 * The CNN half is vpk_cnn_forward: under vpk_cnn_set_range_policy(cnn, 1) the exact recompute of flagged images is part of it
 * and is enqueued before the event that orders the EM behind the CNN, so the EM reads the recomputed maps. */
typedef struct vpk_step_args {
    const uint8_t* sphere;          /* B x sphere_size x sphere_size */
    int32_t batch, sphere_size;
    float* cnn_out;                 /* B x 400: response maps (kept: they are the EM's input) */
    const int64_t* offsets;         /* [host] B + 1 */
    const double* l_in;             /* sum(N) x 3 resident lines (not modified) */
    double* l_work;                 /* sum(N) x 3 working copy, normalised in place by the EM */
    const double* lp;               /* sum(N) x 4 */
    const double* init_vp;          /* NULL or B x n_init x 3 */
    int32_t n_init, max_vp;
    const vpk_em_params* params;
    double* vp_out; double* sigma_out; double* counts_out; double* counts_w_out;
    int32_t* num_vp_out; int64_t* assoc_out; int32_t* iterations_out; int32_t* status_out; uint32_t* flags_out;
    double* records;                /* NULL or B x vpk_record_width() */
    const int64_t* image_ids;       /* device, B (with records) */
    void* events;                   /* NULL or hipEvent_t[4] */
    void* reuse_event;              /* NULL or a hipEvent_t of the caller that guards these buffers: the CNN stream waits
                                       for it before it overwrites cnn_out, and it is recorded behind this step's EM --
                                       so a ring of vpk_step_args can be re-enqueued without host synchronisation */
    const float* em_prior;          /* NULL: the EM's prior is this step's cnn_out (the reference's flow, run_cnn then run_em);
                                       else B x 400 response maps to use instead -- the CNN still runs and still writes
                                       cnn_out (a pipeline whose priors were computed earlier, evaluation.py:285 stores them
                                       in the datum; bench.py's value_fixture_prior) */
} vpk_step_args;
int vpk_pipeline_step(vpk_handle* cnn, vpk_handle* em, const vpk_step_args* a);
/* Fixed-size result records, one row of vpk_record_width() doubles per image: [image id, status, m, (x, y, z) x 20,
 * line count x 20, NaN] with the m <= 20 best-supported VPs in descending order of their counts (calc_horizon.py:34-36:
 * what the horizon selection reads); the records every rank contributes to the final all_gather.
 * What a consumer may rely on: row b is [image_ids[b], status[b], m, ...] whatever the status; num_vp[b] is clamped to
 * [0, max_vp] first and m = min(num_vp, 20); VP k and count k belong together; counts descend, and VPs with EQUAL counts
 * keep their ascending index order (sharding.device_records is the same, bit for bit); everything behind the m-th VP and
 * the m-th count is 0, the last column NaN.
 * What it may NOT rely on: that order among equal counts is not calc_horizon.py:34-36's, which is np.argsort(counts)[::-1]
 * (NumPy's unstable sort, reversed; sharding.pack_records follows it).  Both keep the same VPs with the same counts when
 * m = num_vp; where a run of equal counts straddles the 20th place they may keep different members of the run.  A horizon
 * selected from a record can therefore differ from the one selected from the EM result -- always when every triplet
 * scores 0, since the first three of the order then win.  No path of this library does that: benchmark.py and bench.py
 * select horizons from the EM results of each rank (calculate_horizon_batch) and the gathered records only carry the
 * result; sharding.py never selects one. */
int vpk_record_width(void);
int vpk_build_records(vpk_handle* h, int batch, int max_vp, const int64_t* image_ids, const double* vp,
                      const double* counts, const int32_t* num_vp, const int32_t* status, double* records);

/* ---- fine-grained entry points (single image; unit parity against the reference functions) ---- */
/* calc_lsim (vp_localisation.py:87-108) + line_rating_knn (:34-84) in one pass over the pairs:
 * lsim_out n x n (row stride n), lscore_out n (before the clip), langle_out n (lines_angles). */
int vpk_pairwise(vpk_handle* h, int n, const double* lp, double* lsim_out, double* lscore_out,
                 double* langle_out);
/* find_initial_vps (:111-165) + pdf_params (probability_functions.py:62-96):
 * v0_out num_max x 3, m0_out 1 int32, weights_out 400 fp32. */
int vpk_init_vps(vpk_handle* h, const float* cnn, const uint8_t* sphere, int sphere_size,
                 int num_max, double* v0_out, int32_t* m0_out, float* weights_out);
/* calc_probabilities (probability_functions.py:99-120): v m x 3, s m (floored in place),
 * outputs p_v m, lvsq [m][n], p_vl [m][n], p_l n. */
int vpk_estep(vpk_handle* h, int n, int m, const double* lp, const float* cnn, const double* v,
              double* s, double* p_v_out, double* lvsq_out, double* p_vl_out, double* p_l_out);
/* weight_matrix (vp_localisation.py:515-524): p_vl [m][n], lsim n x n -> w_out [m][n]. */
int vpk_weight_matrix(vpk_handle* h, int n, int m, const double* p_vl, const double* lweight,
                      const double* lsim, double bias, double* w_out);
/* TEST HOOK: calc_probabilities followed by weight_matrix in ONE workgroup, as an iteration of vpk_em_batch runs them: the
 * E-step leaves the smoother's operand panel p_vl * lweight in LDS where its plan allows (M <= 32 and the panel fits the
 * budget) and the smoother consumes it instead of staging one -- the path neither vpk_estep (lweight = 1, panel unread)
 * nor vpk_weight_matrix (no E-step: always staged) reaches.  Inputs as vpk_estep's (lp n x 4, cnn 400, v m x 3, s m floored
 * in place) and vpk_weight_matrix's (lweight n, lsim n x n, bias).  Launched with the LDS budget of vpk_em_batch, so
 * vpk_em_set_lds_panel and vpk_em_set_smoother steer it as they steer the batch.  Outputs: p_vl_out [m][n], w_out [m][n]
 * and info_out, four int32 read from the device functions that decide, after the E-step and before the smoother:
 *   [0] the smoother's plan for m hypotheses (0: no panel, smooth_full in passes or smooth_blocks; 1: smooth_full's panel;
 *       2: the row-sliced panel; 3: the row-sliced kernel in passes),
 *   [1] the panel flag as the E-step left it (0: none; W: smooth_full's [line][W]; 0x100 + W: the row-sliced layout),
 *   [2] 1 when the sparse smoother applies (setting 2, n <= 448, a finite lsim), which then ignores the panel,
 *   [3] VPs per pass: of the row-sliced kernel under plan 3, otherwise of smooth_full (min(32, 8 floor(budget / n / 8))).
 * Not used by any product path. */
int vpk_estep_smooth(vpk_handle* h, int n, int m, const double* lp, const float* cnn, const double* v, double* s,
                     const double* lweight, const double* lsim, double bias, double* p_vl_out, double* w_out,
                     int32_t* info_out);
/* calc_new_vanishing_point (:453-479) for every row of w [m][n]: vp_out m x 3, valid_out m. */
int vpk_mstep(vpk_handle* h, int n, int m, const double* l, const double* w, double* vp_out,
              int32_t* valid_out);
/* TEST HOOK: the whole M-step of one iteration on caller-supplied state -- calc_new_vanishing_point (:453-479), the
 * variance update (:301-307) and the error / removal tests (:309-317; hard mode :353-392) -- through the same device
 * function the batch kernel calls.  w, lvsq, p_vl [m][n]; assoc NULL = soft mode (every line, weights w[m]), else n
 * int32 = hard mode (VP k takes the lines with assoc == k); cur m x 3 = the VPs of the previous iteration.
 * Outputs: vp_out m x 3 and s_out m (rows the M-step does not write keep 0 and -1), err_out m (-1 = none),
 * removed_out m.  Not used by any product path. */
int vpk_mstep_full(vpk_handle* h, int n, int m, const double* l, const double* w, const double* lvsq, const double* p_vl,
                   const int32_t* assoc, const double* cur, double max_stdd, double s_thresh, double* vp_out,
                   double* s_out, double* err_out, int32_t* removed_out);
/* calc_vp_line_counts (:482-512, thresh = 1.96^2 at :248,:419): v m x 3, s m, w [m][n] (the decision metric),
 * lweight n -> counts_out m, counts_w_out m, assoc_out n int64 (-1 = outlier). */
int vpk_line_counts(vpk_handle* h, int n, int m, const double* lp, const double* v, const double* s, const double* w,
                    const double* lweight, double thresh, double* counts_out, double* counts_w_out, int64_t* assoc_out);
/* the clustering inside split_best_vp (:568-578): ldist n x n -> labels n (0/1), flags 1. */
int vpk_cluster2(vpk_handle* h, int n, const double* ldist, int32_t* labels_out,
                 uint32_t* flags_out);

/* ---- the CNN prior outside the EM (batched; asynchronous on the handle's stream) ------------------------ */
/* replaces: pdf_params -- probability_functions.py:62-96 -- for `batch` 20 x 20 float32 response maps at once: keep
 * the 100 strongest cells (:84-87; equal values: the higher index first), divide by their float32 sum (:89) and by
 * float32(2 pi sigma^2) (:90).  sigma = pi / (confidence * 20) (:71) is the caller's, in double; the means (:73-80) do
 * not depend on the map and stay with the caller.  The same device function as the EM's prior (vpk_init_vps'
 * weights_out is this, with confidence 1.282).
 *   cnn batch x 400 fp32 (device, not modified) -> weights_out batch x 400 fp32 (device); an all-zero map gives NaN.
 * batch = 0 does nothing; batch < 0 or sigma <= 0: VPK_ERR_ARG. */
int vpk_prior_params(vpk_handle* h, int batch, const float* cnn, double sigma, float* weights_out);
/* replaces: calc_pdf -- probability_functions.py:8-40 -- the wrapped Gaussian mixture over the (alpha, beta) half
 * sphere, for `batch` mixtures of ncomp components at npts points each; with pts_dim = 3 also calc_angles -- :252-259
 * -- in front of it (what calc_probabilities does for the VPs, :104-105).  One thread per point walks the components in
 * index order, skipping those whose weight is not > 0 (:21), and adds the five exponentials of :22-36 times the weight
 * to one chain (:38): the reference's order of summation.
 *   means    ncomp x 2 fp64 (means_shared != 0) or batch x ncomp x 2 (alpha, beta)
 *   weights  batch x ncomp fp64
 *   pts      npts x pts_dim fp64 (pts_shared != 0) or batch x npts x pts_dim; pts_dim 2: (alpha, beta), 3: VPs (x, y, z)
 *   angles_out  NULL or batch x npts x 2 fp64: the (alpha, beta) the density was taken at
 *   pdf_out  batch x npts fp64
 * All buffers on the device.  batch = 0 or npts = 0 does nothing; negative sizes, sigma <= 0 and pts_dim outside {2, 3}:
 * VPK_ERR_ARG. */
int vpk_mixture_pdf(vpk_handle* h, int batch, int ncomp, const double* means, int means_shared, const double* weights,
                    double sigma, int npts, const double* pts, int pts_dim, int pts_shared, double* angles_out,
                    double* pdf_out);

/* ---- line geometry outside the EM (batched; asynchronous on the handle's stream) ------------------------- */
/* Both entries: lp sum(N) x 4 fp64 (device, not modified), image b's lines are lp[offsets[b] .. offsets[b + 1]); offsets
 * host int64[batch + 1], not decreasing, as vpk_em_batch takes them.  batch = 0 and images without lines do nothing.
 * batch < 0, decreasing offsets and sigma not > 0: VPK_ERR_ARG, nothing is written.  The pair functions are the EM's
 * (vp_localisation.py:700-776: lines_similarity, lines_proximity, lines_points_cosangle with f = 9 -- both callers pass 9,
 * :55 and :701 --, line_distance_closest), with the settings the EM fixes (sigma = 1 at :178, k1 = 10, k2 = 4 at :230) as
 * arguments: the reference's own defaults differ (calc_lsim sigma = 0.1 at :87; line_rating_knn k2 = 3 at :34). */
/* replaces: calc_lsim -- vp_localisation.py:87-108 -- for a batch: per image the symmetric N x N similarity matrix, zero
 * diagonal (:104).  Every unordered pair (i, j < i) is evaluated once as lines_similarity(lp[i], lp[j], sigma) (:106) and
 * stored to both halves (:95-97), so lsim == lsim.T bit for bit; at sigma = 1 the matrix is vpk_pairwise's bit for bit.
 * mat_offsets host int64[batch + 1]: element offset of image b's row-major matrix (row stride N_b) in lsim_out;
 * mat_offsets[b + 1] - mat_offsets[b] >= N_b^2, else VPK_ERR_ARG (the caller may pad; padding is not written).  One launch
 * over (image, block of 16 rows); no distance matrix is written. */
int vpk_line_similarity_batch(vpk_handle* h, int batch, const int64_t* offsets, const double* lp, double sigma,
                              const int64_t* mat_offsets, double* lsim_out);
/* replaces: line_rating_knn -- :34-72, before any clip -- + lines_angles -- :765-776 -- + line_length -- :761 -- for a
 * batch, WITHOUT an N x N matrix: every row's distances (calc_ldist_parfun :75-84, the row itself counts 4) are evaluated
 * on the fly and only the k1 nearest kept; of those the k2 with the largest sharpened cosine (:55-59; equal cosines: the
 * later neighbour first, as argsort(...)[::-1] orders them) give mean(prox * cos) (:61-70).  k1 and k2 are clamped to N_b
 * per image (:40-41) and the divisor is the clamped k2.  Equal distances: the lower index is the nearer.
 *   k1 1..16, k2 1..k1, else VPK_ERR_ARG.  (Up to 16 elements NumPy's argsort is an insertion sort and its order among
 *   equal cosines is defined; k2 > k1 is an IndexError at :63.)
 *   lscore_out / langle_out / llen_out  sum(N) fp64 each (device); any of the three may be NULL and is then not computed
 * At k1 = 10, k2 = 4, sigma = 1 the scores and angles are vpk_pairwise's bit for bit. */
int vpk_line_rating_batch(vpk_handle* h, int batch, const int64_t* offsets, const double* lp, int k1, int k2,
                          double sigma, double* lscore_out, double* langle_out, double* llen_out);

/* ---- VP set maintenance outside the EM (batched; asynchronous on the handle's stream) --------------------- */
/* The three entries run one operation on a caller-supplied VP set per image, one workgroup per image, through the EM
 * workgroup's own device functions.  Images are concatenated: image b's lines are [line_offsets[b], line_offsets[b + 1])
 * and its VPs [vp_offsets[b], vp_offsets[b + 1]) (host int64[batch + 1] each, not decreasing, M_b <= 64 else
 * VPK_ERR_LIMIT before anything is launched); its (M_b x N_b) matrix (row stride N_b) starts at element
 * sum_{a < b} M_a N_a.  Everything else is a device pointer.  batch = 0 does nothing; an image with N_b = 0 or M_b = 0
 * gets no workgroup and none of its outputs is written.  batch < 0, malformed offsets and null buffers: VPK_ERR_ARG, and
 * no output is touched. */
/* replaces: calc_vp_line_counts -- vp_localisation.py:482-512 -- for a batch, under distance_measure "angle"; the other
 * measures: vpk_vp_line_counts_batch_measure below.
 *   lp sum(N) x 4, v sum(M) x 3, s sum(M), metric [m][n] per image, lweights sum(N)
 *   vp_assoc_in  NULL (:486-487: the argmax of the metric over the VPs, first maximum, a NaN counts as the maximum) or
 *                sum(N) int64: entries below 0 skip the line (:494) and come back unchanged; entries of M_b or more
 *                (an IndexError in the reference) skip it and come back as -1.  With it metric may be NULL.
 *   counts_out / counts_w_out sum(M) fp64, vp_assoc_out sum(N) int64 (-1 = outlier :504 or zero weight :506)
 * The outlier test is dist > thresh * sqrt(s[m]) on the caller's s as it stands: where it is false because s[m] is NaN or
 * negative the line counts.  counts_w is a sum in the EM's order (lanes over lines), not the reference's running sum. */
int vpk_vp_line_counts_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets,
                             const double* lp, const double* v, const double* s, const double* metric,
                             const double* lweights, double thresh, const int64_t* vp_assoc_in, double* counts_out,
                             double* counts_w_out, int64_t* vp_assoc_out);
/* replaces: split_best_vp -- vp_localisation.py:527-630, numClusters = 2 -- for a batch, on slice i of the history array.
 *   l sum(N) x 3 (normalised lines), w [m][n] per image (weightMatrix), lweight / langles sum(N), min_diff (:614)
 *   v_out / s_out  (sum(M) + batch) x 3 / (sum(M) + batch): image b's rows start at vp_offsets[b] + b; M_b + 1 rows are
 *                  written, rows past m_out[b] as zeros
 *   m_out batch int32 (M_b or M_b + 1), split_out batch int32 (the VP that was split -- worstVP :561 -- or -1 when the
 *   set is unchanged), flags_out batch uint32 (VPK_EM_FLAG_SPLIT_TIE, _SPLIT_DISCONNECTED, _VP_OVERFLOW)
 *   labels_out  NULL or sum(N) int32: where a worst VP was found (:560), its lines' cluster labels (:578), -1 elsewhere
 * Kept as the reference has them: the in-image test reads VP m, not worstVPs[m] (:557); a cluster of fewer than 3 lines
 * yields no VP and one VP alone changes nothing (:592, :604-617).  A split of a 64-VP set raises VPK_EM_FLAG_VP_OVERFLOW
 * and returns the set as it was.  N_b <= 32768 (VPK_ERR_LIMIT). */
int vpk_vp_split_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets, const double* lp,
                       const double* l, const double* v, const double* s, const double* w, const double* lweight,
                       const double* langles, double min_diff, double* v_out, double* s_out, int32_t* m_out,
                       int32_t* split_out, uint32_t* flags_out, int32_t* labels_out);

/* replaces: merge_vps with calc_angle_to_other_vp -- vp_localisation.py:633-697 -- for a batch, on slice i of the history
 * array, under distance_measure "angle"; the other measures: vpk_vp_merge_batch_measure below.  While the smallest angle between two VPs (the first row-major minimum of the
 * M x M angle matrix, :647-653; the diagonal counts pi) is below thresh: calc_probabilities and weight_matrix of the whole
 * set (:658-659, the EM's E-step and smoother), the new VP k from w[j] + w[k] (:661) and its variance (:663-666), VP j
 * deleted (:674-675).  s[k] is written before the abort test (:666-668): a merge given up because the new VP is None or
 * s[k] > max_stdd returns the changed s[k]; the E-step floors s at 1e-200 in place (probability_functions.py:139).
 *   l sum(N) x 3 (normalised lines), lweight sum(N), lsim per image a plain N_b x N_b matrix (row stride N_b; what
 *   vpk_line_similarity_batch writes) at element lsim_offsets[b] (host int64[batch + 1], at least N_b^2 apart)
 *   prior_weights batch x 400 fp32 and prior_sigma: what vpk_prior_params returns and was given; at most 100 positive
 *   cells are used, as pdf_params leaves them, more raise VPK_VPSET_FLAG_PRIOR_TRUNCATED
 *   v_out sum(M) x 3, s_out sum(M), keep_out sum(M) int32: image b's rows start at vp_offsets[b]; m_out[b] rows are
 *   the merged set and the indices its VPs had in the input, rows past it zeros and -1; m_out, flags_out batch
 * llen, which the reference passes on to calc_probabilities, is read by none of its three calc_lvsq_* and is not taken. */
#define VPK_VPSET_FLAG_PRIOR_TRUNCATED 8u
int vpk_vp_merge_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets, const double* lp,
                       const double* l, const double* v, const double* s, const double* lweight,
                       const int64_t* lsim_offsets, const double* lsim, double wbias, const float* prior_weights,
                       double prior_sigma, double thresh, double max_stdd, double* v_out, double* s_out, int32_t* m_out,
                       int32_t* keep_out, uint32_t* flags_out);

/* replaces: calc_vp_line_counts -- vp_localisation.py:482-512 with its branch on distance_measure (:495-500) -- for a
 * batch.  measure: VPK_DIST_ANGLE, VPK_DIST_DOTPROD or VPK_DIST_AREA (enum vpk_dist_measure below), one kernel each; any
 * other value is VPK_ERR_ARG.  The arguments of vpk_vp_line_counts_batch, and l sum(N) x 3: read by VPK_DIST_DOTPROD only
 * (else it may be NULL; NULL under VPK_DIST_DOTPROD is VPK_ERR_ARG).  The distance is evaluated on v, s and l as they
 * stand (the reference normalises none of them here):
 *   angle    calc_lvsq_single (probability_functions.py:212-224): the bits of vpk_vp_line_counts_batch
 *   dotprod  |v[m] . l[n]| (:496), summed as (l0 v0 + l1 v1) + l2 v2; finite for a VP at infinity
 *   area     calc_lvsq_area_single (probability_functions.py:227-249): vpk_estep_batch's lvsq of the pair
 * A NaN distance makes the outlier test (:504) false and the line counts: under "angle" and "area" for a VP with
 * v[2] == 0, under "area" also where c^2 - b^2 < 0 (:245).  Every argument error is returned before anything is launched
 * and no output is touched. */
int vpk_vp_line_counts_batch_measure(vpk_handle* h, int measure, int batch, const int64_t* line_offsets,
                                     const int64_t* vp_offsets, const double* lp, const double* l, const double* v,
                                     const double* s, const double* metric, const double* lweights, double thresh,
                                     const int64_t* vp_assoc_in, double* counts_out, double* counts_w_out,
                                     int64_t* vp_assoc_out);
/* replaces: merge_vps -- vp_localisation.py:633-684, which hands its distance_measure to calc_probabilities (:658) -- for a
 * batch.  measure as above; the arguments of vpk_vp_merge_batch after it, and its bits under VPK_DIST_ANGLE.  The E-step of
 * every merge round runs under the measure: "dotprod" on l against v as given (calc_lvsq_dotprod,
 * probability_functions.py:150-154), "area" as calc_lvsq_area (:179-209) has it, a NaN where its radicand is negative.
 * max_stdd is the caller's: the EM passes 0.01 under every measure (:339, :448). */
int vpk_vp_merge_batch_measure(vpk_handle* h, int measure, int batch, const int64_t* line_offsets, const int64_t* vp_offsets,
                               const double* lp, const double* l, const double* v, const double* s, const double* lweight,
                               const int64_t* lsim_offsets, const double* lsim, double wbias, const float* prior_weights,
                               double prior_sigma, double thresh, double max_stdd, double* v_out, double* s_out,
                               int32_t* m_out, int32_t* keep_out, uint32_t* flags_out);

/* ---- the E-step outside the EM (batched; asynchronous on the handle's stream) ---------------------------- */
/* replaces: calc_probabilities -- probability_functions.py:99-120 -- after its prior (calc_angles and calc_pdf, :104-105:
 * vpk_mixture_pdf with pts_dim = 3 gives p_v and the angles), with calc_plv (:133-147), calc_pvl (:123-130) and the three
 * distance measures calc_lvsq_angle (:157-176), calc_lvsq_dotprod (:150-154) and calc_lvsq_area (:179-209), for a ragged
 * batch.  Images are concatenated as for the VP set entries above: image b's lines are [line_offsets[b],
 * line_offsets[b + 1]) and its VPs [vp_offsets[b], vp_offsets[b + 1]) (host int64[batch + 1] each, not decreasing, the
 * first not below 0; any M_b); its (M_b x N_b) matrices (row stride N_b) start at element sum_{a < b} M_a N_a.
 * Everything else is a device pointer.
 *   lp  sum(N) x 4     l  sum(N) x 3, read by VPK_DIST_DOTPROD only (else it may be NULL)     v  sum(M) x 3     s  sum(M)
 *   p_v sum(M): the prior of every VP; may be NULL when neither p_l_out nor p_vl_out is given
 *   s_floored_out sum(M): max(s, 1e-200) with a NaN replaced too (:139 writes this into the caller's s; s itself is only read)
 *   lvsq_out / p_lv_out / p_vl_out  [m][n] per image     p_l_out sum(N)
 *   Every output may be NULL and is then not computed.
 * angle: the EM's expression, bit for bit.  dotprod: lv = (l0 v0 + l1 v1) + l2 v2 on v as given.  area: as the reference
 * has it -- np.cross takes the 2-vector v_ as (vx, vy, 0), so the distance is measured from the line through the segment's
 * MIDPOINT in direction v_; a negative radicand at :205 gives NaN.  p_l is one sum over the VPs in ascending order, floored
 * at 1e-12 (:117, a NaN passes).  One thread per line, 64 lines per workgroup, the VPs' values staged 128 at a time; when
 * neither p_l_out nor p_vl_out is given the grid also splits the VP range, and the bits are the same.
 * batch = 0 does nothing; an image with N_b = 0 or M_b = 0 gets no workgroup and none of its outputs is written.  batch < 0,
 * malformed offsets and an unknown measure: VPK_ERR_ARG.  lp, v, s (and l, p_v where the call reads them) are required
 * only when there is work to do -- an image with lines and VPs, and an output that is not NULL: then a null one is
 * VPK_ERR_ARG; a call with nothing to do returns VPK_OK whatever they are.  No error case touches an output. */
enum vpk_dist_measure { VPK_DIST_ANGLE = 0, VPK_DIST_DOTPROD = 1, VPK_DIST_AREA = 2 };
int vpk_estep_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets, const double* lp,
                    const double* l, const double* v, const double* s, const double* p_v, int measure,
                    double* s_floored_out, double* lvsq_out, double* p_lv_out, double* p_l_out, double* p_vl_out);

/* ---- the EM update outside the EM (batched; asynchronous on the handle's stream) -------------------------- */
/* The batched forms of vpk_weight_matrix, vpk_mstep / vpk_mstep_full and vpk_init_vps: one workgroup per image through the
 * same device functions, bit for bit what the single-image entries give image by image.  Conventions as for the VP set
 * entries above: host int64[batch + 1] offsets (not decreasing, the first not below 0), device pointers otherwise, image
 * b's [m][n] matrices (row stride N_b) at element sum_{a < b} M_a N_a.  M_b <= 64 and N_b <= 32768, else VPK_ERR_LIMIT
 * before anything is launched.  batch = 0 does nothing; an image with N_b = 0 or M_b = 0 gets no work and none of its
 * outputs is written.  batch < 0, malformed offsets and a null buffer the call would read or write: VPK_ERR_ARG.  No error
 * case touches an output.
 * The grid is min(images with work, cap) workgroups -- cap: vpk_em_set_workgroups when set, else a small multiple of the
 * CU count -- each with ONE workspace slot sized for the batch's largest image; workgroup q takes the images q, q + grid,
 * ... of a largest-first order.  A workspace beyond half of the device memory: VPK_ERR_LIMIT. */
/* replaces: weight_matrix -- vp_localisation.py:515-524 -- for a batch.
 *   p_vl [m][n] per image, lweight sum(N), lsim / lsim_offsets as vpk_vp_merge_batch takes them (plain N_b x N_b matrices,
 *   at least N_b^2 apart: what vpk_line_similarity_batch writes), w_out [m][n] per image.
 * Launched with the LDS budget of vpk_em_batch: vpk_em_set_lds_panel and vpk_em_set_smoother steer it as they steer
 * vpk_weight_matrix. */
int vpk_weight_matrix_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets,
                            const double* p_vl, const double* lweight, const int64_t* lsim_offsets, const double* lsim,
                            double bias, double* w_out);
/* replaces: calc_new_vanishing_point -- vp_localisation.py:453-479 -- and the variance / error / removal step around it
 * (:284-322 soft, :353-392 hard, with the row normalisation of :358) for a batch.
 *   l sum(N) x 3 (normalised lines), w [m][n] per image
 *   lvsq, p_vl   [m][n] per image; both given or both NULL
 *     both NULL: vpk_mstep -- positions only, from unit state.  s_out, err_out and max_err_out must be NULL; cur and assoc
 *                are not read.
 *     both given: vpk_mstep_full.  assoc NULL = soft; assoc sum(N) int64 (what vpk_vp_line_counts_batch writes) = hard:
 *                entries outside [0, M_b) -- the -1 of an outlier -- select no VP.  cur sum(M) x 3: the VPs of the previous
 *                iteration.  Rows the M-step does not write come back as vp = 0, s = -1, err = -1.
 *   vp_out sum(M) x 3, s_out / err_out sum(M)
 *   removed_out  NULL or sum(M) int32: 1 where the reference appends m to to_be_removed
 *   valid_out    NULL or sum(M) int32: 1 where a new VP was written
 *   max_err_out  NULL or batch fp64: the np.maximum chain from 0 over the image's errors (:275, :313; a NaN sticks) */
int vpk_mstep_batch(vpk_handle* h, int batch, const int64_t* line_offsets, const int64_t* vp_offsets, const double* l,
                    const double* w, const double* lvsq, const double* p_vl, const int64_t* assoc, const double* cur,
                    double max_stdd, double s_thresh, double* vp_out, double* s_out, double* err_out, int32_t* removed_out,
                    int32_t* valid_out, double* max_err_out);
/* replaces: find_initial_vps -- vp_localisation.py:111-165 -- for a batch.
 *   cnn batch x 400 fp32, sphere batch x S x S uint8 (S = sphere_size >= 20), num_max 1..64 (else VPK_ERR_ARG)
 *   v0_out batch x num_max x 3: rows past m0_out[b] are zeros; m0_out batch int32: 0 where the reference raises at :165
 *   weights_out  NULL or batch x 400 fp32: the pdf_params weights, as vpk_init_vps returns them */
int vpk_init_vps_batch(vpk_handle* h, int batch, const float* cnn, const uint8_t* sphere, int sphere_size, int num_max,
                       double* v0_out, int32_t* m0_out, float* weights_out);

/* ---- result overlays (batched; asynchronous on the handle's stream) ---------------------------------------- */
/* Both entries blend primitives into 8-bit RGB images in place, by the renderer of DESIGN section 7d: a primitive of width
 * w covers the points within w / 2 of its closed segment (a capsule; a disc when the segment has no length), coverage of
 * a pixel is counted on its 4 x 4 sub-samples in fp64 with the distance of line_segment_point_distance --
 * vp_localisation.py:743-758 -- before its square root, and with a = floor(255 * coverage * A / 255 + 0.5) every channel
 * becomes (c a + d (255 - a) + 127) / 255 in integers.  The primitives of an image are blended in index order: the order
 * is part of the result.  Pixel (x, y) covers [x, x + 1) x [y, y + 1), row 0 at the top.
 *   pix_offsets   host int64[batch + 1]: image b's bytes start at rgb_inout[pix_offsets[b]], rows of 3 W_b bytes without
 *                 padding; pix_offsets[b + 1] - pix_offsets[b] >= 3 W_b H_b (the caller may pad; padding is not written)
 *   rgb_inout     device; every pixel of an image that has at least one primitive is read and written back (unchanged where
 *                 no primitive reaches it), an image without primitives is not touched, and never a byte outside an image
 *   *_offsets     host int64[batch + 1], not decreasing: image b's primitives are [offsets[b], offsets[b + 1])
 *   *_rgba        device, 4 bytes per primitive (r, g, b, A), 4-byte aligned; opacity = A / 255
 * A primitive with a coordinate or width that is not finite, or a width below 0, is not drawn.  batch = 0 and images
 * without primitives do nothing.  batch < 0, a side below 1 and offsets that do not rise as described: VPK_ERR_ARG, and
 * nothing is launched.  One launch over (image, tile of 16 x 16 pixels), one pixel per thread. */
/* replaces: the ax1.plot calls of show_em_result -- result_plotting.py:93-97 (the lines of the best VPs, lw = 2) and :106-107
 * (the horizon, lw = 10) -- for a batch of images of any sizes.
 *   dims       host int32[2 batch]: W_b, H_b (>= 1)
 *   seg_px     device fp64, sum(P) x 4: end points (px, py, qx, qy) in pixel coordinates (:56-59)
 *   seg_width  device fp64, sum(P): w in pixels */
int vpk_overlay_lines_batch(vpk_handle* h, int batch, const int32_t* dims, const int64_t* pix_offsets, uint8_t* rgb_inout,
                            const int64_t* seg_offsets, const double* seg_px, const uint8_t* seg_rgba,
                            const double* seg_width);
/* replaces: the ax2.plot call of plot_result -- result_plotting.py:135-139 (one round marker per VP, alpha = 0.6) -- for a
 * batch of square panels.
 *   sizes          host int32[batch]: panel b is sizes[b] x sizes[b] pixels (>= 1)
 *   mark_xy        device fp64, sum(P) x 2: centres in pixel coordinates
 *   mark_diameter  device fp64, sum(P): diameters in pixels */
int vpk_overlay_markers_batch(vpk_handle* h, int batch, const int32_t* sizes, const int64_t* pix_offsets,
                              uint8_t* rgb_inout, const int64_t* mark_offsets, const double* mark_xy,
                              const uint8_t* mark_rgba, const double* mark_diameter);

/* diagnostics: y[i] = f(x[i]) for the device's double-precision exp / acos / asin / atan / sqrt / sin / cos / log (fn =
 * 0..7) as the EM kernels call them (same translation unit, same flags).  replaces: nothing -- it measures the premise
 * of the parity bar: the reference's probability_functions.py:99-176 evaluates these through NumPy / libm, and results
 * can only agree to the last bit where these functions do (tests/test_gpu_math.py reports max ulp and mismatch rate). */
int vpk_math_probe(vpk_handle* h, int fn, long long n, const double* x, double* y);

/* ---- horizon from the best orthogonal VP triplet, batched ------------------------------------------ */
/* replaces: calc_horizon.calculate_horizon_and_ortho_vp -- calc_horizon.py:19-225 -- called per image from the
 * scoring loop of benchmark.py:229-243 (maxbest = 20, theta_vmin = pi/10; theta_z = pi/4 at :19).
 *   vp / counts / num_vp  the outputs of vpk_em_batch (B x max_vp x 3, B x max_vp, B; device)
 *   order   B x maxbest int32 (device): np.argsort(counts[:M])[::-1][:maxbest] per image (:34-36); the caller
 *           supplies it because the order of equal counts is a property of its NumPy sort
 *   out     B x 15 fp64 (device): hP1 | hP2 | zVP | hVP1 | hVP2 (3 each), the first five returned values
 *   combo_out  B x 3 int32: best_combo (VP indices; [0,1,-1] / [0,0,-1] in the < 3 VP fallbacks, :200-217) */
int vpk_horizon_batch(vpk_handle* h, int batch, int max_vp, const double* vp, const double* counts,
                      const int32_t* num_vp, const int32_t* order, int maxbest, double theta_vmin, double theta_z,
                      double* out, int32_t* combo_out);

/* ---- detector glue: the order of the best VPs and the conversion to pixels, batched (csrc/detect_device.hpp) -------- */
/* replaces: np.argsort(counts)[::-1][:maxbest] -- calc_horizon.py:34-36 -- for a batch of images on the device, so that
 * vpk_em_batch's outputs reach vpk_horizon_batch without a host round trip.
 *   counts     B x max_vp fp64, num_vp  B int32 (clamped to 0..max_vp as vpk_horizon_batch clamps it): vpk_em_batch's outputs
 *   order_out  B x maxbest int32: the first min(maxbest, M_b) entries are image b's VP indices by descending count, the
 *              entries past that are 0
 * The tie rule is part of the contract: among equal counts the HIGHER index comes first; a NaN count ranks above every
 * number, and among NaNs the higher index comes first.  That is np.argsort(counts, kind="stable")[::-1], and what the
 * reference's NumPy generation gives for up to 16 elements (there its argsort is an insertion sort).  Beyond that the
 * reference's order among equal counts is a property of an unstable sort, so wherever counts tie this rule is the
 * project's own.
 * max_vp and maxbest are 1..64 and batch >= 0, else VPK_ERR_ARG before anything is launched; batch = 0 does nothing.
 * One wave per image, one lane per VP: a lane's rank is the number of VPs that precede it.  Asynchronous on the handle's
 * stream. */
int vpk_vp_order_batch(vpk_handle* h, int batch, int max_vp, const double* counts, const int32_t* num_vp, int maxbest,
                       int32_t* order_out);
/* replaces: the pixel conversion of example.py:66-76 (horizon end points), the inverse of detect_lsd_lines'
 * normalisation (evaluation.py:240-249), for the segments, the VPs and the horizon of a batch of images.  With
 * scale = max(w, h):   x_px = x * scale / 2.0 + w / 2.0    y_px = -y * scale / 2.0 + h / 2.0
 * evaluated left to right in fp64, each operation rounded on its own (no FMA): NumPy's bytes.
 *   dims          [host] B x 2 int32: width, height of the detector image, as vpk_lsd_rows_to_lines takes it
 *   line_offsets  [host] B+1 int64 prefix sums of the segment counts; lp  sum(N) x 4 fp64 normalised segments
 *   vp / num_vp   B x max_vp x 3 fp64, B int32: vpk_em_batch's outputs (max_vp 1..64; num_vp clamped to 0..max_vp)
 *   horizon       B x 15 fp64: vpk_horizon_batch's `out`
 *   lp_px_out       sum(N) x 4 fp64, rows as in lp
 *   vp_px_out       B x max_vp x 2 fp64: (v[0] / v[2], v[1] / v[2]) in pixels -- a VP at infinity gives the infinities
 *                   and NaNs IEEE gives; rows at or past num_vp[b] are written as NaN
 *   horizon_px_out  B x 2 x 2 fp64: hP1 and hP2 (x, y) in pixels
 * Each output may be NULL (not written; its inputs are then not read and may be NULL).  A side below 1, decreasing
 * offsets, batch < 0 and a missing input of a requested output: VPK_ERR_ARG, nothing is launched.  batch = 0 does
 * nothing.  One thread per output row.  Asynchronous on the handle's stream. */
int vpk_to_pixels_batch(vpk_handle* h, int batch, const int32_t* dims, const int64_t* line_offsets, const double* lp,
                        int max_vp, const double* vp, const int32_t* num_vp, const double* horizon, double* lp_px_out,
                        double* vp_px_out, double* horizon_px_out);

/* ---- scoring: horizon errors against ground truth and their AUC, batched (csrc/score_device.hpp) -------------------- */
/* replaces: the error of one image -- benchmark.py:245-253 -- for a batch:
 *   thP1 = np.cross(trueHorizon, [1, 0, 1]);  thP2 = np.cross(trueHorizon, [-1, 0, 1]);  thP /= thP[2]       (:248-251)
 *   max_error = np.maximum(|hP1[1] - thP1[1]|, |hP2[1] - thP2[1]|) / 2 * scale * 1.0 / imageHeight            (:253)
 * with scale = max(w, h) (:137).  The value is NumPy's byte for byte: the cross products are written out as NumPy
 * evaluates a 3-vector cross product (each product and each difference rounds on its own, no FMA), the rest runs left to
 * right in fp64, and maximum hands a NaN on.
 *   horizon       B x 15 fp64: vpk_horizon_batch's `out` (hP1 at 0..2, hP2 at 3..5)
 *   true_horizon  B x 3 fp64: the ground-truth horizon line in the normalised frame
 *   dims          [host] B x 2 int32: width, height of the image file, as vpk_to_pixels_batch takes it
 *   err_out       B fp64
 * batch < 0, a null buffer and a side below 1: VPK_ERR_ARG, nothing is launched.  batch = 0 does nothing.  One thread per
 * image.  Asynchronous on the handle's stream. */
int vpk_horizon_error_batch(vpk_handle* h, int batch, const double* horizon, const double* true_horizon, const int32_t* dims,
                            double* err_out);
/* replaces: auc.calc_auc -- auc.py:5-37, called at benchmark.py:264 -- on a device vector of n errors.
 *   sorted_out  n fp64: the errors in np.sort's order, ascending with NaN last (must not be `err`)
 *   auc_out     1 fp64 (device): the area under (err[i], (i + 1) / n) up to `cutoff`, divided by the cutoff
 * A NaN error counts in the fractions and never falls under the cutoff.  `mid` is auc.py:20-28's: strict < on both sides
 * of the cutoff, the last crossing wins.  The tail point (cutoff, 1 or mid) follows np.argsort(kind="stable"): a data
 * point whose error equals the cutoff comes before it.  (Beyond 16 points the reference's own argsort is unstable, so
 * there this rule is the project's.)  The order comes from a rank by counting -- thread i counts the errors that precede
 * error i, equal errors told apart by index -- and the trapezoid sum from ONE workgroup in a fixed order, without
 * floating-point atomics: the same input gives the same bits on every run.  The sum's order is not np.trapz's pairwise one:
 * the two agree within 2 (n + 4) 2^-53.
 * n < 1: VPK_ERR_ARG (the reference indexes plot_points[-1]); n > 65536: VPK_ERR_LIMIT; a null buffer: VPK_ERR_ARG;
 * nothing is launched.  Asynchronous on the handle's stream. */
int vpk_auc(vpk_handle* h, int n, const double* err, double cutoff, double* sorted_out, double* auc_out);

/* ---- fine-tuning the dense head: train/train_val.prototxt:289-417 under train/solver.prototxt -------------------------
 * The trainer keeps fp32 master copies of fc6 [H6 x I], fc7 [H7 x H6] and fc8 [O x H7] with their biases, a momentum
 * buffer for each, and the activations of one step.  It is separate from the forward's packed weights: a trained head
 * reaches a forward through vpk_train_store and vpk_cnn_load.  The conv stack below is frozen: the input X is
 * vpk_cnn_forward_tap's tap 7 (pool5), B x I in Caffe's C x H x W order.
 *
 * The solver's numbers; vpk_train_default_params sets the prototxts' values. */
typedef struct vpk_train_params {
    float base_lr;            /* solver.prototxt:8   1e-4 */
    float gamma;              /* :10  0.1; lr = base_lr * gamma^floor(iteration / stepsize) (lr_policy "step", :9) */
    int64_t stepsize;         /* :11  200000 */
    float momentum;           /* :17  0.9 */
    float weight_decay;       /* :18  5e-4 */
    float lr_mult_weight;     /* train_val.prototxt:295, 335, 375   1 */
    float decay_mult_weight;  /* :296, 336, 376   1 */
    float lr_mult_bias;       /* :299, 339, 379   2 */
    float decay_mult_bias;    /* :300, 340, 380   0 */
    float dropout_ratio;      /* :326, 366   0.5 */
} vpk_train_params;
void vpk_train_default_params(vpk_train_params* p);
/* dims = (I, H6, H7, O), all >= 1 (else VPK_ERR_ARG); the net's are (57600, 4096, 4096, 400).  Allocates weights, momentum,
 * activations and the backward's workspace; one trainer per handle (a second create: VPK_ERR_STATE).  vpk_destroy frees it. */
int vpk_train_create(vpk_handle* h, const int32_t dims[4]);
int vpk_train_destroy(vpk_handle* h);
/* dropout_ratio in [0, 1) and stepsize >= 1, else VPK_ERR_ARG.  Takes effect with the next step. */
int vpk_train_set_params(vpk_handle* h, const vpk_train_params* p);
/* blobs [host]: fp32 fc6 weight, fc6 bias, fc7 weight, fc7 bias, fc8 weight, fc8 bias -- the last six of vpk_cnn_load's.
 * vpk_train_load zeroes the momentum and the iteration counter (a solver started from a caffemodel);
 * vpk_train_load_momentum / vpk_train_store_momentum move the momentum in the same layout (the history of a solverstate).
 * All four wait for the handle's stream.  Before vpk_train_load the other three return VPK_ERR_STATE. */
int vpk_train_load(vpk_handle* h, const void* const blobs[6]);
int vpk_train_store(vpk_handle* h, void* const blobs_out[6]);
int vpk_train_load_momentum(vpk_handle* h, const void* const blobs[6]);
int vpk_train_store_momentum(vpk_handle* h, void* const blobs_out[6]);
/* the solver's iteration: it selects the learning rate (solver.prototxt:8-11) and keys the generated dropout masks */
int vpk_train_set_iteration(vpk_handle* h, long long iteration);
int vpk_train_get_iteration(const vpk_handle* h, long long* iteration_out);
/* One solver iteration on a batch of 1 <= B <= 32 rows (the prototxt's batch size is 5, train_val.prototxt:14); B outside that
 * range: VPK_ERR_LIMIT before anything is launched, the state is unchanged.  All pointers are device pointers.
 *   forward (TRAIN phase, :289-393)  a6 = relu(X W6^T + b6), d6 = a6 m6 / (1 - p); the same for fc7; z = d7 W8^T + b8
 *   loss (:411-417)  sum over B x O of max(z,0) - z t + log1p(exp(-|z|)), divided by B; dz = (sigmoid(z) - t) / B
 *   backward         dW = dY^T X, db = sum_b dY, dX = dY W through dropout and ReLU; no dX below fc6
 *   update (solver.prototxt:1, 17, 18)  V <- momentum V + lr_local (dW + decay_local W), W <- W - V
 *   X          B x I fp32          labels  B x O fp32 in [0, 1]
 *   mask6/7    B x H6 / B x H7 uint8 0/1 keep masks, both or neither (else VPK_ERR_ARG).  NULL: generated from
 *              (seed, iteration, layer, b, j) by the counter-based hash documented in csrc/train_device.hpp
 *   loss_out   1 fp32 (may be NULL)    sigout_out  B x O fp32: sigmoid(z), the prototxt's sigout (:419-424; may be NULL)
 * Each layer's weights are read once by the forward, and read and written once, with their momentum, by a fused
 * backward-and-update sweep; no float atomics, so the same state and inputs give the same bits.  Asynchronous on the
 * handle's stream; increments the iteration. */
int vpk_train_step(vpk_handle* h, const float* X, const float* labels, int B, const uint8_t* mask6, const uint8_t* mask7,
                   unsigned long long seed, float* loss_out, float* sigout_out);
/* The TEST phase of the same net (:289-424 without Dropout's mask and scale) on any B >= 1, in chunks of 32; changes no
 * weight.  labels may be NULL (then loss_out is not written); with labels, loss_out is required.  The loss is divided by B. */
int vpk_train_eval(vpk_handle* h, const float* X, const float* labels, int B, float* loss_out, float* sigout_out);
/* vpk_train_step that also writes dX_out [B x I fp32, required]: the gradient of the loss with respect to X (dA6 W6, with
 * the weights the forward used).  The weights, the loss and sigout get the bits vpk_train_step gives them.  The fc6
 * sweep's dX partials (row tiles x B x I floats) are allocated by the first such call and grown when B grows. */
int vpk_train_step_dx(vpk_handle* h, const float* X, const float* labels, int B, const uint8_t* mask6, const uint8_t* mask7,
                      unsigned long long seed, float* loss_out, float* sigout_out, float* dX_out);

/* ---- fine-tuning the conv stack: train/train_val.prototxt:66-288 under train/solver.prototxt ---------------------------
 * A stack is an input shape (C, H, W) and a chain of layers of three kinds.  Fields a kind does not name are ignored.
 *   VPK_LAYER_CONV  out_channels, kernel, stride (>= 1), pad (>= 0), groups, relu.  Cross-correlation with OIHW weights
 *                   [OC][C / groups][K][K] on contiguous channel groups, then the bias, then max(., 0) if relu != 0.
 *                   Output side (in + 2 pad - K) / stride + 1.
 *   VPK_LAYER_LRN   local_size (n, odd), alpha, beta, k.  ACROSS_CHANNELS: s_i = k + (alpha / n) sum x_j^2 over the
 *                   channels |j - i| <= n / 2 that exist, in rising j; y_i = x_i s_i^-beta.
 *   VPK_LAYER_POOL  kernel, stride.  MAX over the window [o stride, min(o stride + K, in)) with Caffe's ceil-mode output
 *                   side ceil((in - K) / stride) + 1 (in >= K; less one if the last window would start past the plane).  The maximum is the first element in row-major scan order
 *                   that is strictly greater than all before it; its flat index h W + w in the input plane is kept. */
enum { VPK_LAYER_CONV = 0, VPK_LAYER_LRN = 1, VPK_LAYER_POOL = 2 };
typedef struct vpk_stack_layer {
    int32_t kind;
    int32_t out_channels, kernel, stride, pad, groups, relu;
    int32_t local_size;
    float alpha, beta, k;
} vpk_stack_layer;
/* The net's own stack (conv1, norm1, pool1, conv2, norm2, pool2, conv3, conv4, conv5, pool5 on (1, 500, 500)): writes up to
 * `capacity` layers and in_shape[3] (either may be NULL) and returns the number of layers, 10.  Needs no handle. */
int vpk_convtrain_net_layers(vpk_stack_layer* layers_out, int capacity, int32_t in_shape[3]);
/* One conv trainer per handle (a second create: VPK_ERR_STATE), beside the head trainer.  Shapes that do not chain are
 * VPK_ERR_ARG before anything is allocated: a non-positive size or output side, groups that do not divide both channel
 * counts, an even local_size, a pool larger than its plane, n_layers outside 1..32; an LRN on more than 512 channels:
 * VPK_ERR_LIMIT.  Allocates the fp32 master weights and momentum of every CONV layer; the blobs of a step are allocated
 * by the first forward of a batch size and kept.  vpk_destroy frees it. */
int vpk_convtrain_create(vpk_handle* h, int C, int H, int W, const vpk_stack_layer* layers, int n_layers);
int vpk_convtrain_destroy(vpk_handle* h);
/* The solver's numbers (dropout_ratio is ignored); stepsize >= 1, else VPK_ERR_ARG. */
int vpk_convtrain_set_params(vpk_handle* h, const vpk_train_params* p);
/* blobs [host]: two fp32 blobs per CONV layer in stack order, weight then bias.  The rules of vpk_train_load and its kin. */
int vpk_convtrain_load(vpk_handle* h, const void* const* blobs);
int vpk_convtrain_store(vpk_handle* h, void* const* blobs_out);
int vpk_convtrain_load_momentum(vpk_handle* h, const void* const* blobs);
int vpk_convtrain_store_momentum(vpk_handle* h, void* const* blobs_out);
int vpk_convtrain_set_iteration(vpk_handle* h, long long iteration);
int vpk_convtrain_get_iteration(const vpk_handle* h, long long* iteration_out);
/* The forward of the stack on X [device, B x C x H x W fp32], 1 <= B <= 32 (else VPK_ERR_LIMIT, nothing is launched).
 * X is copied; every layer's output, every LRN's s and every pool's indices stay on the device until the next forward.
 * top_out (may be NULL) receives the last blob, B x C' x H' x W'.  VPK_ERR_STATE before vpk_convtrain_load. */
int vpk_convtrain_forward(vpk_handle* h, const float* X, int B, float* top_out);
/* d_top [device]: dL / d(last blob) for the batch of the last forward (VPK_ERR_STATE without one; a backward consumes it).
 * Back-propagates through every layer (ReLU by top > 0; pools by a gather over the windows that contain an element, in
 * row-major window order; LRN dx_i = dy_i s_i^-beta - (2 alpha beta / n) x_i sum_j dy_j y_j / s_j; convolutions dW, db
 * and, for every CONV layer but the first, dX), applies V <- mu V + lr_local (dW + decay_local W), W <- W - V to every
 * CONV layer with vpk_train_step's rate arithmetic, and increments the iteration.  d_input_out (may be NULL): B x C x H x W,
 * dL / dX; NULL skips the first layer's data gradient.  The weight gradient's reduction over (b, y, x) runs on the f32
 * matrix cores in slabs whose sums are added in slab order inside the update: no float atomics, the same state and inputs
 * give the same bits.  The gradient blob of every layer stays on the device until the next forward. */
int vpk_convtrain_backward(vpk_handle* h, const float* d_top, float* d_input_out);
/* Copies one kept blob of `layer`, dense, to out [device]: VPK_BLOB_OUTPUT fp32, VPK_BLOB_POOL_INDEX int32 (POOL layers),
 * VPK_BLOB_GRADIENT fp32 (dL / d output, after a backward), VPK_BLOB_LRN_SCALE fp32 (LRN layers: s, Caffe's scale_ blob).
 * A kind the layer does not have: VPK_ERR_ARG; a blob that does not exist yet: VPK_ERR_STATE. */
enum { VPK_BLOB_OUTPUT = 0, VPK_BLOB_POOL_INDEX = 1, VPK_BLOB_GRADIENT = 2, VPK_BLOB_LRN_SCALE = 3 };
int vpk_convtrain_read(vpk_handle* h, int layer, int kind, void* out);

/* ---- the training set on the device: train/train_val.prototxt:1-62 without LMDB ------------------------------------------
 * stands in for: the two Data layers of train_val.prototxt:1-62 (TRAIN batch 5, TEST batch 100, mean_file).  A stored
 * example is an image's homogeneous lines and its ground-truth VPs; a batch is gathered from the store, mapped by one affine
 * transform of the image plane per example, and handed to vpk_sphere_raster (l_out, out_offsets) and to the loss
 * (labels_out).  The rules are csrc/trainset_device.hpp's, fp64, every operation rounded on its own:
 *   H = [[h00, h01, h02], [h10, h11, h12], [0, 0, 1]];  det = h00 h11 - h01 h10
 *   line  mx = h11 lx - h10 ly;  my = h00 ly - h01 lx;  mz = det lz - (h02 mx + h12 my)       (det H^-T l)
 *   VP    wx = (h00 vx + h01 vy) + h02 vz;  wy = (h10 vx + h11 vy) + h12 vz;  wz = vz            (H v)
 *   cell  the VP normalised and flipped into z >= 0, point_to_angle, angle_to_index on (gh, gw), floor(. + 0.5) on both
 *         axes (coordinate_conversion.py:23-35, 53-61); -1 for a zero or non-finite VP and for a cell outside the map
 *   l [device] sum(N) x 3 fp64 and line_offsets [host] n + 1 int64: the store's lines (vpk_lsd_rows_to_lines' l_out)
 *   vps [device] sum(V) x 3 fp64 and vp_offsets [host] n + 1 int64: its ground-truth VPs
 *   index [host] B int32 in 0..n-1, repeats allowed; transforms [host] B x 6 fp64 (h00 h01 h02 h10 h11 h12), NULL: the
 *   identity, and then l_out is the stored lines byte for byte; out_offsets [host] B + 1 int64: the prefix sums of the
 *   chosen images' line counts (checked); gh, gw 1..64.
 *   Outputs [device], each may be NULL: l_out sum x 3 fp64; vp_out sum(V_b) x 3 fp64 in batch order; cell_out int32 per
 *   VP (a gw + b or -1); labels_out B x gh gw fp32, zeroed by the call, 1.0f in every VP's cell (plain stores).
 * Only the B indexed entries of the store's host offsets are read, and O(B) words are uploaded.  Asynchronous on the
 * handle's stream.  VPK_ERR_ARG before anything is launched or written: a null handle, null offsets / index / out_offsets,
 * null l or vps that an output needs, n < 1, B < 1, an index outside 0..n-1, out_offsets that do not match, a non-finite
 * transform or det == 0, gh or gw outside 1..64. */
int vpk_trainset_batch(vpk_handle* h, const double* l, const int64_t* line_offsets, const double* vps, const int64_t* vp_offsets,
                       int n, const int32_t* index, const double* transforms, int B, const int64_t* out_offsets, int gh, int gw,
                       double* l_out, double* vp_out, int32_t* cell_out, float* labels_out);
/* stands in for: transform_param.mean_file (train_val.prototxt:1-62; Caffe's compute_image_mean).  Adds B uint8 rasters of P
 * pixels [device, B x P] into sum [device, P uint32], one thread per pixel, images in index order: integer sums, exact.
 * count [host]: the images summed so far, in and out; a call that would take it past floor((2^32 - 1) / 255) = 16 843 009
 * returns VPK_ERR_LIMIT and adds nothing.  B < 1, P < 1, a negative count or a null buffer: VPK_ERR_ARG.  Asynchronous. */
int vpk_trainset_accumulate(vpk_handle* h, const uint8_t* rasters, int B, int64_t P, uint32_t* sum, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* VPK_H_ */
