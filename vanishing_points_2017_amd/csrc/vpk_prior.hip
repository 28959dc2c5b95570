// vpk_prior.hip -- the CNN prior outside the EM: batched pdf_params and the mixture density at caller-supplied points
// (vpk_prior_params, vpk_mixture_pdf; see include/vpk.h).  The arithmetic is prior_device.hpp's, which the EM workgroup
// uses too.  Compiled with -ffp-contract=off like the EM unit.
#include "prior_device.hpp"
#include "vpk_internal.hpp"

using namespace vpk;

namespace {

constexpr int PARAMS_THREADS = 512;   // one round over the 400 cells
constexpr size_t PARAMS_LDS_BYTES = ((2 * NCELL + 1) * sizeof(float) + 15) / 16 * 16;

// one workgroup per map: prior_setup's rule (keep 100, f32 pairwise sum, two f32 divisions) without the EM context
__global__ __launch_bounds__(PARAMS_THREADS) void prior_params_kernel(const float* cnn, double sigma, float* weights_out) {
    float* wts = reinterpret_cast<float*>(lds_base());
    float* keep = wts + NCELL;
    const size_t b = (size_t)block_id();
    prior_keep_sum((cgfp)cnn + b * NCELL, wts, keep);
    const float sum = keep[NCELL];
    const float dv = prior_norm_f32(sigma);
    for (int i = tid(); i < NCELL; i += nthreads()) weights_out[b * NCELL + i] = prior_weight(keep[i], sum, dv);
}

// one workgroup (one wave) per tile of PRIOR_TILE points of one image; the block index is image-major
template <int DIM> __global__ __launch_bounds__(PRIOR_TILE) void mixture_pdf_kernel(MixtureArgs a, int tiles) {
    mixture_pdf_tile<DIM>(a, block_id() / tiles, block_id() % tiles);
}

}  // namespace

extern "C" {

int vpk_prior_params(vpk_handle* h, int batch, const float* cnn, double sigma, float* weights_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0 || !(sigma > 0)) return vpk_fail(h, VPK_ERR_ARG, "vpk_prior_params: bad argument");
    if (batch == 0) return VPK_OK;
    if (!cnn || !weights_out) return vpk_fail(h, VPK_ERR_ARG, "vpk_prior_params: null buffer");
    VPK_HIP(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(prior_params_kernel, dim3((unsigned)batch), dim3(PARAMS_THREADS), PARAMS_LDS_BYTES, h->stream, cnn, sigma,
                       weights_out);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

int vpk_mixture_pdf(vpk_handle* h, int batch, int ncomp, const double* means, int means_shared, const double* weights,
                    double sigma, int npts, const double* pts, int pts_dim, int pts_shared, double* angles_out,
                    double* pdf_out) {
    if (!h) return VPK_ERR_ARG;
    if (batch < 0 || ncomp < 0 || npts < 0 || !(sigma > 0) || (pts_dim != 2 && pts_dim != 3))
        return vpk_fail(h, VPK_ERR_ARG, "vpk_mixture_pdf: bad argument");
    if (batch == 0 || npts == 0) return VPK_OK;
    if ((ncomp > 0 && (!means || !weights)) || !pts || !pdf_out)
        return vpk_fail(h, VPK_ERR_ARG, "vpk_mixture_pdf: null buffer");
    const int tiles = (npts + PRIOR_TILE - 1) / PRIOR_TILE;
    if ((long long)tiles * batch > 0x7fffffffLL) return vpk_fail(h, VPK_ERR_ARG, "vpk_mixture_pdf: batch x npts too large for one launch");
    MixtureArgs a;
    a.ncomp = ncomp; a.npts = npts;
    a.means = (cgdp)means; a.means_stride = means_shared ? 0 : 2LL * ncomp;
    a.weights = (cgdp)weights;
    a.kk = -0.5 / (sigma * sigma);                 // probability_functions.py:34
    a.pts = (cgdp)pts; a.pts_stride = pts_shared ? 0 : (long long)pts_dim * npts;
    a.angles_out = (gdp)angles_out; a.pdf_out = (gdp)pdf_out;
    VPK_HIP(h, hipSetDevice(h->device));
    const dim3 grid((unsigned)(tiles * batch));
    if (pts_dim == 3)
        hipLaunchKernelGGL(mixture_pdf_kernel<3>, grid, dim3(PRIOR_TILE), PRIOR_LDS_BYTES, h->stream, a, tiles);
    else
        hipLaunchKernelGGL(mixture_pdf_kernel<2>, grid, dim3(PRIOR_TILE), PRIOR_LDS_BYTES, h->stream, a, tiles);
    VPK_HIP(h, hipGetLastError());
    return VPK_OK;
}

}  // extern "C"
