// pm_driver.cpp -- TEST-ONLY: the portable elementary functions of csrc/lsd_portable_math.hpp (the GPU line segment
// detector's test math policy) over arrays, for tests/test_lsd_portable_math.py.  Built with -ffp-contract=off like
// every unit that includes the header.
#include "../../vanishing_points_2017_amd/csrc/lsd_portable_math.hpp"

// out[i] = f(a[i]) or f(a[i], b[i]): fn 0 atan2(a, b), 1 sin, 2 cos, 3 exp, 4 log, 5 log10, 6 pow(a, b), 7 sinh
extern "C" int pm_eval(int fn, long long n, const double* a, const double* b, double* out) {
    for (long long i = 0; i < n; ++i) {
        const double x = a[i];
        switch (fn) {
            case 0: out[i] = vpk_pmath::atan2(x, b[i]); break;
            case 1: out[i] = vpk_pmath::sin(x); break;
            case 2: out[i] = vpk_pmath::cos(x); break;
            case 3: out[i] = vpk_pmath::exp(x); break;
            case 4: out[i] = vpk_pmath::log(x); break;
            case 5: out[i] = vpk_pmath::log10(x); break;
            case 6: out[i] = vpk_pmath::pow(x, b[i]); break;
            case 7: out[i] = vpk_pmath::sinh(x); break;
            default: return -1;
        }
    }
    return 0;
}
