"""Hand-made inputs of the E-step for the tests that hold its three-pass form (the responsibilities that are zero left out,
csrc/em_estep.hpp) to the dense form vpk_em_set_smoother(h, 1) keeps: shared by tests/test_em_estep_zeros.py (the host build)
and tests/test_gpu_em_estep_zeros.py (the kernels).  Nothing here is an expected value: the two forms are compared with
each other, output for output, bit for bit.

Shapes.  N = 12, 64, 65, 130, 257: on the GPU 8, 4, 2, 2 lanes per line and one lane per line with a ragged fifth wave (the
host build has one lane).  M = 1, 3, 4, 5, 8, 9: below, at and above the four-deep unroll and the VP tile of 8; M = 33 and 64:
no panel is planned above 32 VPs, so both settings take the dense loop there.

Variants, each met by every shape:
    mixed     variances from the 1e-200 floor (given as 1e-300) over both measures' max_stdd (1e-6, 1e-3) to 1e-2, the scene's own
              VPs among the hypotheses: kept and left-out terms side by side in every line
    small_s   every variance tiny: lines whose terms ALL underflow (p_l on its 1e-12 floor)
    big_s     every variance at max_stdd of "dotprod" or wider: under "dotprod" nothing underflows, every VP is kept
    inf_vp    mixed, the first VP with a zero third coordinate: a NaN column under "angle", which makes every p_l NaN
    nan_map   mixed, a NaN cell in the response map: every weight of the prior is NaN, and prior_setup lists only the cells whose
              weight is > 0 -- none: every p_v is +0.0, every term (0.0 included: exp * k2 * 0.0) is zero, every p_l on its floor.
              (No response map makes a p_v NaN here: the listed weights are finite and positive and a component's sum of
              exponentials is at most 5.  The next variant makes one through the VP.)
    nan_pv    mixed, the second VP off the unit sphere (|y| > 1: asin is NaN): that VP's p_v alone is NaN, its lvsq is finite
"""
import numpy as np

SHAPES_N = (12, 64, 65, 130, 257)
SHAPES_M = (1, 3, 4, 5, 8, 9, 33, 64)
VARIANTS = ("mixed", "small_s", "big_s", "inf_vp", "nan_map", "nan_pv")
S_MIXED = (1e-300, 1.2e-7, 1e-6, 1e-4, 1e-3, 1e-2)
S_SMALL = (1e-300, 1e-12, 1.2e-7)
S_BIG = (1e-3, 1e-2, 1.0)

_cache = {}


def case(n, m, variant):
    """{"l" (n,3) unit, "lp" (n,4), "cnn" (20,20) f32, "v" (m,3), "s" (m), "lweight" (n), "lsim" (n,n)}.  Made once per
    (n, m, variant); nobody writes into what this returns."""
    key = (n, m, variant)
    if key in _cache:
        return _cache[key]
    from vanishing_points_2017_amd import synth
    seed = 1000 * n + m
    rs = np.random.RandomState(seed)
    sc = synth.make_scene(seed, max(n, 12), 3)
    lp = sc["lp"][:n].copy()
    if n >= 7:
        lp[2, 2:] = lp[2, :2]                               # a zero-length segment: its direction's norm is 0
        lp[3] = (0.3, -0.2, 0.3 + 1e-3, -0.2 + 0.7e-3)      # a short segment that points at none of the hypotheses
    l = sc["l"][:n].copy()
    l /= np.sqrt((l * l).sum(1))[:, None]
    v = rs.randn(m, 3)
    v[:, 2] = np.abs(v[:, 2]) + 0.05
    tv = np.asarray(sc["true_vps"], dtype=np.float64)
    k = min(m, tv.shape[0])
    v[m - k:] = tv[:k]                                      # lines that point at them: terms that do not underflow
    v /= np.sqrt((v * v).sum(1))[:, None]
    table = {"small_s": S_SMALL, "big_s": S_BIG}.get(variant, S_MIXED)
    s = np.array([table[(i + n) % len(table)] for i in range(m)])
    cnn = sc["cnn_response"].astype(np.float32).copy()
    if variant == "inf_vp":
        v[0] = (0.6, 0.8, 0.0)
    elif variant == "nan_map":
        cnn.reshape(-1)[int(np.argmax(cnn))] = np.nan
    elif variant == "nan_pv":
        v[min(1, m - 1)] = (0.3, 1.5, 0.5)
    lweight = rs.uniform(0.0, 1.0, n)
    lweight[::7] = 0.0
    lsim = rs.uniform(0.0, 1.0, (n, n))
    lsim = 0.5 * (lsim + lsim.T)
    _cache[key] = {"l": l, "lp": lp, "cnn": cnn, "v": v, "s": s, "lweight": lweight, "lsim": lsim}
    return _cache[key]


def all_cases():
    return [(n, m, var) for n in SHAPES_N for m in SHAPES_M for var in VARIANTS]


def same_bits(a, b, keys):
    """array_equal on the values AND on the sign of zero; a NaN matches a NaN"""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, k
        assert np.array_equal(x, y, equal_nan=True), k
        if x.dtype.kind == "f":
            num = ~np.isnan(x)
            assert np.array_equal(np.signbit(x[num]), np.signbit(y[num])), k + " (sign)"
