// sim_overlay.cpp -- TEST-ONLY host build of csrc/overlay_device.hpp (unmodified; see hip_sim.hpp): the tiles of
// vpk_overlay_lines_batch and vpk_overlay_markers_batch, which on the GPU are workgroups of 256 threads with one pixel each,
// run one after the other here with one lane that takes the tile's 256 pixels in turn (and stages a chunk of primitives in
// 256 rounds of one).  It is not a product path: nothing in the package builds, loads or links it.
#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/overlay_device.hpp"

using namespace vpk;

extern "C" {

// dims: batch x (W, H); the other arguments as the library's entry points take them (include/vpk.h), all in host memory
int sim_overlay(int disc, int batch, const long long* dims, const long long* pix_offsets, unsigned char* rgb,
                const long long* prim_offsets, const double* geom, const unsigned char* rgba, const double* width) {
    static_assert(OV_LDS_BYTES <= sizeof(g_sim_lds), "the tile's LDS does not fit the simulated LDS");
    OverlayArgs a = {};
    a.dims = dims; a.pix_offsets = pix_offsets; a.prim_offsets = prim_offsets;
    a.geom = geom; a.width = width; a.rgba = reinterpret_cast<const unsigned*>(rgba); a.rgb = rgb;
    long long tmax = 0;     // as the launch: the largest image's tiles for every image, those past an image's own return at once
    for (int b = 0; b < batch; ++b) {
        const long long tiles = ((dims[2 * b] + OV_TILE - 1) / OV_TILE) * ((dims[2 * b + 1] + OV_TILE - 1) / OV_TILE);
        if (tiles > tmax) tmax = tiles;
    }
    for (int b = 0; b < batch; ++b)
        for (int t = 0; t < tmax; ++t) {
            if (disc) overlay_tile<true>(a, b, t);
            else overlay_tile<false>(a, b, t);
        }
    return 0;
}

}  // extern "C"
