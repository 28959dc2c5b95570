// sim_estep.cpp -- TEST-ONLY host build of csrc/estep_device.hpp (unmodified; see hip_sim.hpp): the workgroups of
// vpk_estep_batch run one after the other here with one lane each (ESTEP_TILE = WAVE = 1: a tile is one line), found through
// the same block table and the same search as on the GPU.  It is not a product path: nothing in the package builds, loads
// or links it.
#include <vector>

#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/estep_device.hpp"

using namespace vpk;

extern "C" {

// split: -1 = as the library chooses (split when neither p_l nor p_vl is asked for), 0 / 1 = forced (1 needs both null)
int sim_estep_batch(int batch, const long long* line_off, const long long* vp_off, const double* lp, const double* l,
                    const double* v, const double* s, const double* p_v, int measure, int split, double* s_out,
                    double* lvsq_out, double* p_lv_out, double* p_l_out, double* p_vl_out) {
    const bool chain = p_l_out || p_vl_out;
    if (split < 0) split = chain ? 0 : 1;
    if (split && chain) return -1;
    std::vector<long long> mat(batch + 1), blk(batch + 1);
    long long mt = 0, bk = 0;
    for (int b = 0; b < batch; ++b) {
        const long long n = line_off[b + 1] - line_off[b], m = vp_off[b + 1] - vp_off[b];
        mat[b] = mt; blk[b] = bk;
        mt += n * m;
        bk += estep_image_blocks(n, m, split != 0);
    }
    mat[batch] = mt; blk[batch] = bk;
    EstepArgs a = {};
    a.batch = batch; a.split = split;
    a.line_off = line_off; a.vp_off = vp_off; a.mat_off = mat.data(); a.blk_off = blk.data();
    a.lp = lp; a.l = l; a.v = v; a.s = s; a.p_v = p_v;
    a.s_out = s_out; a.lvsq_out = lvsq_out; a.p_lv_out = p_lv_out; a.p_l_out = p_l_out; a.p_vl_out = p_vl_out;
    for (long long k = 0; k < bk; ++k) {
        if (measure == VPK_DIST_ANGLE) estep_block<VPK_DIST_ANGLE>(a, k);
        else if (measure == VPK_DIST_DOTPROD) estep_block<VPK_DIST_DOTPROD>(a, k);
        else if (measure == VPK_DIST_AREA) estep_block<VPK_DIST_AREA>(a, k);
        else return -1;
    }
    return 0;
}

}  // extern "C"
