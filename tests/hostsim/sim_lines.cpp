// sim_lines.cpp -- TEST-ONLY host build of csrc/line_device.hpp (unmodified; see hip_sim.hpp): the row blocks of
// vpk_line_similarity_batch and the rows of vpk_line_rating_batch, which on the GPU are workgroups, run one after the
// other here with one lane each (a tile is then 16 rows x 1 column and a rating workgroup holds one row).  It is not a
// product path: nothing in the package builds, loads or links it.
#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/line_device.hpp"

using namespace vpk;

extern "C" {

int sim_line_similarity(int batch, const long long* offsets, const double* lp, double sigma, const long long* mat_offsets,
                        double* lsim_out) {
    LineBatchArgs a = {};
    a.offsets = offsets; a.mat_offsets = mat_offsets; a.lp = lp; a.sigma = sigma; a.lsim = lsim_out;
    for (int b = 0; b < batch; ++b) {
        const long long n = offsets[b + 1] - offsets[b];
        for (int blk = 0; blk < (n + LS_RB - 1) / LS_RB; ++blk) line_similarity_rowblock(a, b, blk);
    }
    return 0;
}

// lds_lines: images of at most this many lines take the staged path (their lp copied in front of the walk)
int sim_line_rating(int batch, const long long* offsets, const double* lp, int k1, int k2, double sigma, double* lscore_out,
                    double* langle_out, double* llen_out, int lds_lines) {
    LineBatchArgs a = {};
    a.offsets = offsets; a.lp = lp; a.sigma = sigma; a.k1 = k1; a.k2 = k2;
    a.lscore = lscore_out; a.langle = langle_out; a.llen = llen_out; a.lds_lines = lds_lines;
    if ((size_t)(LR_KS + 4 * (size_t)lds_lines) * sizeof(double) > sizeof(g_sim_lds)) return -1;
    for (int b = 0; b < batch; ++b) {
        const long long n = offsets[b + 1] - offsets[b];
        for (int blk = 0; blk < n; ++blk) line_rating_block(a, b, blk);
    }
    return 0;
}

}  // extern "C"
