// vpk_internal.hpp -- host-side state shared by the translation units of libvpk.so
#ifndef VPK_INTERNAL_HPP_
#define VPK_INTERNAL_HPP_

#include <vector>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>

#include "../../include/vpk.h"
#include "em_layout.hpp"

struct vpk_cnn_state;   // vpk_cnn.hip
struct vpk_train_state; // vpk_train.hip
struct vpk_convtrain_state; // vpk_convtrain.hip

// a device header uploaded through pinned staging.  The device buffer is one, rewritten in stream order; the staging is a ring
// of `depth` pinned buffers, each reused once the event of the upload that last left it has fired, so a caller waits only for
// the copy issued `depth` calls ago (vpk_stage_begin / vpk_stage_commit)
struct vpk_staged {
    static constexpr int MAX_RING = 4;
    int depth = 1;
    int cur = 0;                 // the ring slot of the next upload
    struct { void* host; size_t bytes; hipEvent_t ev; bool ev_valid; } ring[MAX_RING] = {};
    void* dev = nullptr;
    size_t dev_bytes = 0;
};

struct vpk_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    int num_cu = 0;
    int cu_share = 0;            // CUs this handle's launches are sized for (= num_cu)
    int em_max_workgroups = 0;   // vpk_em_set_workgroups (0 = no cap)
    int em_smoother = 0;         // vpk_em_set_smoother
    int em_lds_doubles = 0;      // vpk_em_set_lds_panel (0 = whole CU)
    int em_measure = 0;          // vpk_em_set_distance_measure (VPK_DIST_ANGLE)
    // capacities of the time-sliced launches' parked-image lists (vpk_em.hip); the environment variables
    // VPK_EM_WAIT_CAP / VPK_EM_STARTED_CAP shrink them at vpk_create so that tests can fill them with a few images
    int em_wait_cap = 8192;
    int em_started_cap = 1024;
    int lds_per_block = 0;
    int arch = 0;
    size_t total_mem = 0;
    // EM workspace (grown on demand, never shrunk)
    void* em_ws = nullptr;
    size_t em_ws_bytes = 0;
    vpk_staged em_hdr = {vpk_staged::MAX_RING};   // offsets + order + queue counter; vpk_em_batch never waits for the previous batch
    void* small_ws = nullptr; // fine-grained entry points
    size_t small_ws_bytes = 0;
    bool raster_ready = false;
    void* raster_hdr = nullptr;
    size_t raster_hdr_bytes = 0;
    std::vector<long long> raster_offsets;   // the offsets the device copy in raster_hdr holds (same batch again: no upload, no wait)
    int raster_table_size = 0;               // canvas size the sample table in raster_hdr was made for
    int raster_last_batch = 0;               // batch of the last vpk_sphere_raster call (vpk_sphere_raster_flags' layout)
    int raster_alternative = 0;              // vpk_sphere_raster_set_alternative
    bool em_ready = false;    // dynamic-LDS attribute set on the EM kernels
    // time-sliced EM launches (vpk_em_set_time_slice): images not finished within a launch's budget are parked
    // in device-side lists and resumed by the next launch; their slots outlive the launch
    double em_slice_ms = 0.0;        // 0 = off: every call runs its images to completion
    vpk_em_dist_out em_dist = {};    // vpk_em_set_distribution_out: outputs of the next vpk_em_batch call
    bool em_dist_set = false;
    int em_slice_nmax = 0;           // slots are sized for at least this many lines
    void* em_sess = nullptr;         // [counters | slot flags | parked-image list A | list B]
    size_t em_sess_bytes = 0;
    int em_sess_in = 0;              // which list the next launch drains
    bool em_unflushed = false;       // parked images may exist
    size_t em_sess_slot_bytes = 0;   // geometry the parked images were laid out with
    int em_sess_slots = 0;
    int em_sess_wgs = 0;
    int em_sess_wt_doubles = 0;
    size_t em_sess_lds = 0;
    vpk::EmLayout em_sess_layout = {};
    hipEvent_t step_event = nullptr; // vpk_pipeline_step: orders the EM stream behind the CNN stream
    vpk_cnn_state* cnn = nullptr;
    // vpk_lsd_detect_batch (vpk_lsd_gpu.hip): workspace (grown on demand), header (descriptors + Gaussian weights)
    size_t lsd_ws_limit = 0;         // vpk_lsd_set_workspace_limit (0 = the default, 4 GiB)
    int lsd_math = 0;                // vpk_lsd_set_math (test hook): 0 = device libm, 1 = portable math
    void* lsd_ws = nullptr;
    size_t lsd_ws_bytes = 0;
    vpk_staged lsd_hdr;
    // vpk_image_prepare_batch / vpk_lsd_rows_to_lines (vpk_frontend.hip): headers (descriptors + Lanczos weights) and the
    // horizontal pass's uint8 intermediate (grown on demand)
    vpk_staged fe_prep, fe_rows;
    void* fe_ws = nullptr;
    size_t fe_ws_bytes = 0;
    vpk_staged lines_hdr;            // vpk_line_similarity_batch / vpk_line_rating_batch (vpk_lines.hip): the offsets
    vpk_staged overlay_hdr;          // vpk_overlay_lines_batch / vpk_overlay_markers_batch (vpk_overlay.hip): sizes + offsets
    vpk_staged vpset_hdr;            // vpk_vp_line_counts_batch / vpk_vp_split_batch (vpk_vpset.hip): offsets + active images
    void* vpset_ws = nullptr;        // their per-image workspace (grown on demand)
    size_t vpset_ws_bytes = 0;
    bool vpset_ready = false;        // dynamic-LDS attribute set on the kernel
    vpk_staged estep_hdr;            // vpk_estep_batch (vpk_estep.hip): offsets of lines, VPs, matrices and workgroups
    vpk_staged emstep_hdr;           // vpk_weight_matrix_batch / vpk_mstep_batch (vpk_emstep.hip): the image records
    void* emstep_ws = nullptr;       // one slot per workgroup (grown on demand)
    size_t emstep_ws_bytes = 0;
    bool emstep_ready = false;       // dynamic-LDS attribute set on the kernel
    vpk_staged detect_hdr;           // vpk_to_pixels_batch (vpk_detect.hip): line offsets + image sizes
    vpk_staged score_hdr;            // vpk_horizon_error_batch (vpk_score.hip): image sizes
    vpk_staged trainset_hdr = {vpk_staged::MAX_RING};   // vpk_trainset_batch (vpk_trainset.hip): offsets + transforms of one batch
    vpk_train_state* train = nullptr; // vpk_train_create (vpk_train.hip): the dense head's master weights, momentum, activations
    vpk_convtrain_state* convtrain = nullptr; // vpk_convtrain_create (vpk_convtrain.hip): the conv stack's weights, momentum, blobs
};

int vpk_fail(vpk_handle* h, int code, const char* what);
int vpk_fail_hip(vpk_handle* h, hipError_t e, const char* what);
int vpk_reserve(vpk_handle* h, void** p, size_t* have, size_t want, const char* what);
void vpk_cnn_free(vpk_handle* h);
void vpk_train_free(vpk_handle* h);
void vpk_convtrain_free(vpk_handle* h);
// An upload to s.dev through s's pinned staging, asynchronously on the handle's stream.  begin: the next ring slot, free of
// its last upload and at least `bytes` large, as *host; the caller fills it.  commit: s.dev reserved for bytes + tail (the tail
// is not written), the copy of `bytes`, the slot's event.  vpk_stage_upload: begin, memcpy of src, commit.
int vpk_stage_begin(vpk_handle* h, vpk_staged& s, size_t bytes, void** host);
int vpk_stage_commit(vpk_handle* h, vpk_staged& s, size_t bytes, const char* what, size_t tail = 0);
int vpk_stage_upload(vpk_handle* h, vpk_staged& s, const void* src, size_t bytes, const char* what);

#define VPK_HIP(h, call)                                         \
    do {                                                         \
        hipError_t e_ = (call);                                  \
        if (e_ != hipSuccess) return vpk_fail_hip(h, e_, #call); \
    } while (0)

#endif
