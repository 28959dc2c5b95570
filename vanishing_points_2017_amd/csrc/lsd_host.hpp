// lsd_host.hpp -- the line segment detector for one image on the host: the functions of lsd_device.hpp run serially with a
// one-lane wave.  detect_image<Libm> is vpk_lsd_detect (vpk_lsd.cpp); detect_image<Portable> is the host side of the
// bit-for-bit pin of the GPU batch (tests/hostsim/sim_lsd.cpp).  What the GPU batch does in five kernels
// (vpk_lsd_gpu.hip) are the loops here.  Plain C++: no HIP, no handle.
#ifndef VPK_LSD_HOST_HPP_
#define VPK_LSD_HOST_HPP_

#include <vector>

#include "lsd_device.hpp"

namespace vpk_lsd {

struct HostWave {
    int lane() const { return 0; }
    int size() const { return 1; }
    int sum_int(int v) const { return v; }
    double max_d(double v) const { return v; }
    double min_d(double v) const { return v; }
};

// image: width x height grey levels.  Rows go to out (max_segments of 7 doubles); *n_out is the full count, which may
// exceed max_segments: call again with a larger buffer.  Returns 0, or -1 for an argument it cannot run on.
template <class M>
int detect_image(const double* image, int width, int height, double scale, double* out, int max_segments, int* n_out) {
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
    // the seeds: defined pixels, bins high to low, column-major within a bin (what lsd_order sorts on the GPU)
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

}  // namespace vpk_lsd

#endif
