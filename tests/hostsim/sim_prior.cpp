// sim_prior.cpp -- TEST-ONLY host build of csrc/prior_device.hpp (unmodified; see hip_sim.hpp): the tiles of
// vpk_mixture_pdf and the maps of vpk_prior_params, which on the GPU are workgroups, run one after the other here with
// one lane each.  It is not a product path: nothing in the package builds, loads or links it.
#include "hip_sim.hpp"
#include "../../vanishing_points_2017_amd/csrc/prior_device.hpp"

using namespace vpk;

extern "C" {

int sim_prior_params(int batch, const float* cnn, double sigma, float* weights_out) {
    float* wts = reinterpret_cast<float*>(lds_base());
    float* keep = wts + NCELL;
    for (int b = 0; b < batch; ++b) {
        prior_keep_sum(cnn + (size_t)b * NCELL, wts, keep);
        const float dv = prior_norm_f32(sigma);
        for (int i = 0; i < NCELL; ++i) weights_out[(size_t)b * NCELL + i] = prior_weight(keep[i], keep[NCELL], dv);
    }
    return 0;
}

int sim_mixture_pdf(int batch, int ncomp, const double* means, int means_shared, const double* weights, double sigma, int npts,
                    const double* pts, int pts_dim, int pts_shared, double* angles_out, double* pdf_out) {
    MixtureArgs a;
    a.ncomp = ncomp; a.npts = npts;
    a.means = means; a.means_stride = means_shared ? 0 : 2LL * ncomp;
    a.weights = weights;
    a.kk = -0.5 / (sigma * sigma);
    a.pts = pts; a.pts_stride = pts_shared ? 0 : (long long)pts_dim * npts;
    a.angles_out = angles_out; a.pdf_out = pdf_out;
    const int tiles = (npts + PRIOR_TILE - 1) / PRIOR_TILE;
    for (int b = 0; b < batch; ++b)
        for (int t = 0; t < tiles; ++t) {
            if (pts_dim == 3) mixture_pdf_tile<3>(a, b, t);
            else mixture_pdf_tile<2>(a, b, t);
        }
    return 0;
}

}  // extern "C"
