// overlay_device.hpp -- result overlays: coloured line segments and discs blended into RGB images, the per-pixel work of
// the reference's result_plotting.py (ax1.plot at :97 and :107, ax2.plot at :138-139).  The renderer is specified in
// DESIGN section 7d (colour, capsule coverage on 4 x 4 sub-samples, integer blend, draw order); this file is that
// specification as device code.
//
// One user: the two kernels of vpk_overlay.hip, whose body is overlay_tile at the end of this file.  Written against the
// vocabulary of wave_prims.hpp only, so that tests/hostsim/sim_overlay.cpp compiles it unmodified with g++ (hip_sim.hpp: one
// lane, WAVE = 1; the lane then walks the 256 pixels of a tile one after the other).  The distance is line_device.hpp's
// seg_point_dist_sq -- line_segment_point_distance, vp_localisation.py:743-758, before its square root -- and the unit is
// compiled with -ffp-contract=off like the other users of that header.
// Citations are file:line under the reference tree.
#ifndef VPK_OVERLAY_DEVICE_HPP_
#define VPK_OVERLAY_DEVICE_HPP_

#include "line_device.hpp"

namespace vpk {

typedef VPK_GLOBAL unsigned char* gbp;
typedef const VPK_GLOBAL unsigned* cgup;

struct OverlayArgs {
    cglp dims;           // [2 batch]: image b is dims[2 b] = W pixels wide and dims[2 b + 1] = H high
    cglp pix_offsets;    // [batch + 1]: image b's bytes are rgb[pix_offsets[b] ..), rows of 3 W bytes
    cglp prim_offsets;   // [batch + 1]: image b's primitives are [prim_offsets[b], prim_offsets[b + 1]), in draw order
    cgdp geom;           // segments: sum(P) x 4 (px, py, qx, qy); discs: sum(P) x 2 (centre), pixel coordinates
    cgdp width;          // sum(P): width of the segment / diameter of the disc, pixels
    cgup rgba;           // sum(P): bytes r, g, b, A in memory order; opacity = A / 255
    gbp rgb;             // the images, blended in place
};

constexpr int OV_TILE = 16;                          // a workgroup's tile: 16 x 16 pixels
constexpr int OV_PIX = OV_TILE * OV_TILE;
constexpr int OV_CHUNK = 256;                        // primitives staged per round
constexpr int OV_THREADS = WAVE == 64 ? 256 : 1;     // one pixel per thread; the host build's single lane takes all 256
constexpr int OV_PPT = OV_PIX / OV_THREADS;          // pixels per thread
constexpr int OV_NF = 9;                             // doubles per staged primitive: x1 y1 x2 y2 dx dy nn | (w/2)^2 | reach^2
constexpr int OV_MAX_WAVES = 4;
constexpr size_t OV_LDS_BYTES = (size_t)OV_CHUNK * (OV_NF * sizeof(double) + sizeof(unsigned)) + OV_MAX_WAVES * sizeof(int);

VPK_DEV bool ov_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and +-inf

// squared distance from (px, py) to the closed segment; a segment without length is its end point (a disc when inflated):
// the reference's quotient (:748) is 0 / 0 there
VPK_DEV double ov_dist_sq(const LineGeom& s, double px, double py) {
    if (!(s.nn > 0)) {
        const double ex = s.x1 - px, ey = s.y1 - py;
        return dot2(ex, ey, ex, ey);
    }
    return seg_point_dist_sq(s, px, py);
}

// d' = (c a + d (255 - a) + 127) / 255 per channel (blend)
VPK_DEV unsigned ov_blend(unsigned c, unsigned d, unsigned a) { return (c * a + d * (255u - a) + 127u) / 255u; }

// One 16 x 16 tile of one image, by one workgroup: every primitive of the image, in draw order, over every pixel of the tile.
//
// The primitives pass through LDS in chunks of OV_CHUNK.  Each thread takes one primitive of the chunk, derives what every
// pixel needs of it (the LineGeom, (w/2)^2 and the squared reach of a pixel centre) and tests its bounding box, inflated by
// w / 2, against the tile; the survivors are written to LDS compacted IN ORDER (wave ballot + prefix over the lanes below,
// the waves' counts through LDS), because the blend does not commute.  Then every pixel walks the survivors: a primitive
// whose distance from the pixel centre exceeds w / 2 + 0.75 cannot hold one of the pixel's sub-samples (those lie within
// sqrt(2) * 0.375 = 0.53 of the centre) and is skipped after one distance; otherwise the 16 sub-samples are counted and
// the pixel is blended in integers.  The pixel's three bytes are read once in front of the first chunk and written once
// behind the last; a tile of an image without primitives returns without touching memory.
// A primitive with a coordinate or width that is not finite, or a width below 0, is not drawn.
template <bool DISC>
VPK_DEV void overlay_tile(const OverlayArgs& A, int img, int tile) {
    const int W = uniform_int((int)A.dims[2 * img]), H = uniform_int((int)A.dims[2 * img + 1]);
    const int ntx = (W + OV_TILE - 1) / OV_TILE, nty = (H + OV_TILE - 1) / OV_TILE;
    if ((long long)tile >= (long long)ntx * nty) return;
    const long long p0 = A.prim_offsets[img];
    const int P = uniform_int((int)(A.prim_offsets[img + 1] - p0));
    if (P <= 0) return;
    const int x0 = (tile % ntx) * OV_TILE, y0 = (tile / ntx) * OV_TILE;
    const double tx1 = (double)x0 + OV_TILE, ty1 = (double)y0 + OV_TILE;   // in double: x0 + 16 leaves int for a side near 2^31
    gbp image = A.rgb + A.pix_offsets[img];
    double* f = reinterpret_cast<double*>(lds_base());
    unsigned* col = reinterpret_cast<unsigned*>(f + OV_NF * OV_CHUNK);
    int* wcnt = reinterpret_cast<int*>(col + OV_CHUNK);

    unsigned cr[OV_PPT], cg[OV_PPT], cb[OV_PPT];
#pragma unroll
    for (int u = 0; u < OV_PPT; ++u) {
        const int p = tid() + u * OV_THREADS, x = x0 + (p & (OV_TILE - 1)), y = y0 + p / OV_TILE;
        cr[u] = cg[u] = cb[u] = 0;
        if (x < W && y < H) {
            const size_t at = ((size_t)y * W + x) * 3;
            cr[u] = image[at]; cg[u] = image[at + 1]; cb[u] = image[at + 2];
        }
    }

    for (int c0 = 0; c0 < P; c0 += OV_CHUNK) {
        int count = 0;                                              // survivors of this chunk (the same in every thread)
        for (int r0 = 0; r0 < OV_CHUNK; r0 += OV_THREADS) {         // one trip on the GPU
            const int i = c0 + r0 + tid();
            bool keep = false;
            double a[4] = {0, 0, 0, 0}, w = 0;
            if (i < P) {
                const size_t e = (size_t)(p0 + i);
                if (DISC) {
                    a[0] = a[2] = A.geom[2 * e]; a[1] = a[3] = A.geom[2 * e + 1];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) a[q] = A.geom[4 * e + q];
                }
                w = A.width[e];
                const double hw = w / 2;
                const double lox = a[0] < a[2] ? a[0] : a[2], hix = a[0] < a[2] ? a[2] : a[0];
                const double loy = a[1] < a[3] ? a[1] : a[3], hiy = a[1] < a[3] ? a[3] : a[1];
                keep = ov_finite(a[0]) && ov_finite(a[1]) && ov_finite(a[2]) && ov_finite(a[3]) && ov_finite(w) && w >= 0 &&
                       lox - hw <= tx1 && hix + hw >= x0 && loy - hw <= ty1 && hiy + hw >= y0;
            }
            const unsigned long long bal = wave_ballot(keep);
            if (lane() == 0) wcnt[wave_id()] = popcount64(bal);
            block_sync();
            int base = count;
            for (int v = 0; v < nwaves(); ++v) {
                const int c = wcnt[v];
                base += v < wave_id() ? c : 0;
                count += c;
            }
            if (keep) {
                const int s = base + popcount64(bal & lanes_below());
                const LineGeom g = line_geom(a);
                const double hw = w / 2, reach = hw + 0.75;
                f[0 * OV_CHUNK + s] = g.x1; f[1 * OV_CHUNK + s] = g.y1; f[2 * OV_CHUNK + s] = g.x2; f[3 * OV_CHUNK + s] = g.y2;
                f[4 * OV_CHUNK + s] = g.dx; f[5 * OV_CHUNK + s] = g.dy; f[6 * OV_CHUNK + s] = g.nn;
                f[7 * OV_CHUNK + s] = hw * hw; f[8 * OV_CHUNK + s] = reach * reach;
                col[s] = A.rgba[(size_t)(p0 + i)];
            }
            block_sync();                                           // the list is complete; wcnt may be written again
        }
#pragma unroll
        for (int u = 0; u < OV_PPT; ++u) {
            const int p = tid() + u * OV_THREADS, x = x0 + (p & (OV_TILE - 1)), y = y0 + p / OV_TILE;
            if (!(x < W && y < H)) continue;
            for (int s = 0; s < count; ++s) {
                LineGeom g;
                g.x1 = f[0 * OV_CHUNK + s]; g.y1 = f[1 * OV_CHUNK + s]; g.x2 = f[2 * OV_CHUNK + s]; g.y2 = f[3 * OV_CHUNK + s];
                g.dx = f[4 * OV_CHUNK + s]; g.dy = f[5 * OV_CHUNK + s]; g.nn = f[6 * OV_CHUNK + s];
                g.vx = g.vy = g.nv = 0;
                const double rr = f[7 * OV_CHUNK + s];
                if (!(ov_dist_sq(g, x + 0.5, y + 0.5) <= f[8 * OV_CHUNK + s])) continue;
                int k = 0;
                for (int j = 0; j < 4; ++j) {
                    const double sy = y + (0.125 + 0.25 * j);       // (j + 0.5) / 4, exact
#pragma unroll
                    for (int q = 0; q < 4; ++q) k += ov_dist_sq(g, x + (0.125 + 0.25 * q), sy) <= rr ? 1 : 0;
                }
                if (k == 0) continue;
                const unsigned c = col[s];
                const double opacity = (double)(c >> 24) / 255.0;
                const unsigned al = (unsigned)floor(255.0 * (k / 16.0) * opacity + 0.5);
                cr[u] = ov_blend(c & 255u, cr[u], al);
                cg[u] = ov_blend((c >> 8) & 255u, cg[u], al);
                cb[u] = ov_blend((c >> 16) & 255u, cb[u], al);
            }
        }
        block_sync();                                               // the next chunk overwrites the list
    }

#pragma unroll
    for (int u = 0; u < OV_PPT; ++u) {
        const int p = tid() + u * OV_THREADS, x = x0 + (p & (OV_TILE - 1)), y = y0 + p / OV_TILE;
        if (x < W && y < H) {
            const size_t at = ((size_t)y * W + x) * 3;
            image[at] = (unsigned char)cr[u]; image[at + 1] = (unsigned char)cg[u]; image[at + 2] = (unsigned char)cb[u];
        }
    }
}

}  // namespace vpk
#endif
