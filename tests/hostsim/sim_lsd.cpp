// sim_lsd.cpp -- TEST-ONLY host build of the GPU line segment detector's arithmetic (csrc/lsd_device.hpp, unmodified):
// the Gaussian samples, the gradient, the seed bins and the region stage are the product's code, run with glibc's libm and
// a one-lane wave; only the orchestration around them -- five kernels over a batch on the GPU, the LDS counting sort of
// lsd_order -- is a serial loop here.  tests/test_hostsim_lsd.py checks it bit for bit against vpk_lsd_detect.
// sim_lsd_portable is the same with the portable math policy (lsd_portable_math.hpp): the rows the GPU must reproduce
// byte for byte under vpk_lsd_set_math(h, 1) (tests/test_gpu_lsd_exact.py).
// It is not a product path: nothing in the package builds, loads or links it.
#include "../../vanishing_points_2017_amd/csrc/lsd_device.hpp"

#include <vector>

using namespace vpk_lsd;

namespace {

struct HostWave {
    int lane() const { return 0; }
    int size() const { return 1; }
    int sum_int(int v) const { return v; }
    double max_d(double v) const { return v; }
    double min_d(double v) const { return v; }
};

template <class M>
int run(const double* image, int width, int height, double scale, double* out, int max_segments, int* n_out) {
    if (!image || width < 8 || height < 8 || !n_out || max_segments < 0 || (max_segments > 0 && !out) || !(scale > 0.0))
        return -1;
    const Params q = make_params(scale);
    int xs, ys;
    scaled_size(width, height, scale, xs, ys);
    std::vector<double> scaled;
    const double* img = image;
    if (scale != 1.0) {
        const int count = xs > ys ? xs : ys;
        std::vector<double> wt((size_t)count * q.taps), aux((size_t)xs * height);
        gaussian_weights(wt.data(), count, q);
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < xs; ++x)
                aux[(size_t)y * xs + x] = sample(image + (size_t)y * width, width, 1, x, &wt[(size_t)x * q.taps], q);
        scaled.resize((size_t)xs * ys);
        for (int y = 0; y < ys; ++y)
            for (int x = 0; x < xs; ++x)
                scaled[(size_t)y * xs + x] = sample(aux.data() + x, height, xs, y, &wt[(size_t)y * q.taps], q);
        img = scaled.data();
    }
    std::vector<double> angles((size_t)xs * ys), modgrad((size_t)xs * ys);
    double max_grad = 0.0;
    for (int y = 0; y < ys; ++y)
        for (int x = 0; x < xs; ++x) {
            double a;
            const double g = gradient<M>(img, xs, ys, x, y, q.rho, &a);
            angles[(size_t)y * xs + x] = a;
            modgrad[(size_t)y * xs + x] = g;
            if (a != NOTDEF && g > max_grad) max_grad = g;
        }
    // the seeds lsd_order produces: defined pixels, bins high to low, column-major within a bin
    std::vector<std::vector<int>> bins(N_BINS);
    if (max_grad > 0.0)
        for (int x = 0; x < xs - 1; ++x)
            for (int y = 0; y < ys - 1; ++y) {
                const size_t adr = (size_t)y * xs + x;
                if (angles[adr] != NOTDEF) bins[grad_bin(modgrad[adr], max_grad)].push_back((int)adr);
            }
    std::vector<int> order;
    for (int i = N_BINS - 1; i >= 0; --i) order.insert(order.end(), bins[i].begin(), bins[i].end());
    std::vector<unsigned char> used((size_t)xs * ys, 0);
    std::vector<Pt> reg((size_t)xs * ys);
    const HostWave w;
    const double logNT = log_nt(xs, ys);
    const Region<HostWave, M> r{w, angles.data(), modgrad.data(), used.data(), reg.data(), xs, ys, logNT};
    *n_out = r.detect(order.data(), (int)order.size(), q, min_reg_size(logNT, q.p), out, max_segments);
    return 0;
}

}  // namespace

extern "C" int sim_lsd(const double* image, int width, int height, double scale, double* out, int max_segments, int* n_out) {
    return run<Libm>(image, width, height, scale, out, max_segments, n_out);
}

extern "C" int sim_lsd_portable(const double* image, int width, int height, double scale, double* out, int max_segments,
                                int* n_out) {
    return run<Portable>(image, width, height, scale, out, max_segments, n_out);
}
