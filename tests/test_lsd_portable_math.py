"""The portable elementary functions of csrc/lsd_portable_math.hpp -- the test-only math policy under which the GPU line
segment detector is pinned bit for bit against its host build (tests/test_gpu_lsd_exact.py) -- against mpmath at 50
digits, on about 1e5 arguments per function drawn over what the detector feeds them, plus the edge values.  The bounds
are the header's: 2 ulp for atan2, sin, cos, exp, log; 4 ulp for log10, pow, sinh.  Also: the C99 special values and
finite, deterministic results outside those domains."""
import ctypes
import math

import numpy as np
import pytest

from hostsim import hostbuild

mpmath = pytest.importorskip("mpmath")

N = 100000
FN = {"atan2": 0, "sin": 1, "cos": 2, "exp": 3, "log": 4, "log10": 5, "pow": 6, "sinh": 7}
BOUND = {"atan2": 2, "sin": 2, "cos": 2, "exp": 2, "log": 2, "log10": 4, "pow": 4, "sinh": 4}
PI = math.pi
TINY = 5e-324


@pytest.fixture(scope="module")
def pm():
    lib = hostbuild.load("pm")
    lib.pm_eval.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def run(name, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.zeros_like(a) if b is None else np.ascontiguousarray(np.broadcast_to(b, a.shape), dtype=np.float64)
        out = np.empty_like(a)
        assert lib.pm_eval(FN[name], a.size, a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p),
                           out.ctypes.data_as(ctypes.c_void_p)) == 0
        return out
    return run


def _exact(name, a, b):
    mp = mpmath
    x = mp.mpf(float(a))
    if name == "atan2":
        if x == 0:                                             # C99: the signs of the zeros pick 0 or pi
            return mp.mpf(0) if math.copysign(1.0, b) > 0 else mp.pi * math.copysign(1.0, a)
        return mp.atan2(x, mp.mpf(float(b)))
    if name == "pow":
        return x ** int(b)
    return getattr(mp, name)(x)


def _ulps(name, got, a, b):
    """|got - exact| in units of the last place of the exact value (2^-1074 among the subnormals)."""
    err = np.empty(got.size)
    with mpmath.workdps(50):
        for i in range(got.size):
            ref = _exact(name, a[i], b[i] if b is not None else None)
            if ref == 0:
                err[i] = 0.0 if got[i] == 0 else np.inf
                continue
            e = mpmath.frexp(ref)[1] - 1                       # 2^e <= |ref| < 2^(e + 1)
            ulp = mpmath.ldexp(1, max(e, -1022) - 52)
            err[i] = float(abs(mpmath.mpf(float(got[i])) - ref) / ulp)
    return err


def _args(name):
    """(a, b) over the detector's domain of `name` plus its edge values."""
    rs = np.random.RandomState(FN[name] + 100)
    b = None
    if name == "atan2":
        k = N // 5
        y, x = rs.uniform(-1e3, 1e3, 3 * k), rs.uniform(-1e3, 1e3, 3 * k)     # gradients, inertia moments
        ang, rad = rs.uniform(-PI, PI, k), 10.0 ** rs.uniform(-300, 300, k)  # every direction, every scale
        y, x = np.r_[y, rad * np.sin(ang)], np.r_[x, rad * np.cos(ang)]
        base = rs.uniform(-1e3, 1e3, k)                                        # close to the axes
        small = base * 10.0 ** rs.uniform(-25, 0, k) * rs.choice([-1, 1], k)
        flip = rs.rand(k) < 0.5
        y, x = np.r_[y, np.where(flip, small, base)], np.r_[x, np.where(flip, base, small)]
        edge_y = [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 1.0, 1.0, -1.0, -1.0, 1e-300, -1e-300, TINY, 3.0, 1e300]
        edge_x = [1.0, 1.0, -1.0, -1.0, 0.0, 0.0, -0.0, 5.0, 1.0, -1.0, 1.0, -1.0, -1.0, -1.0, -TINY, -0.0, 1e-300]
        return np.r_[y, edge_y], np.r_[x, edge_x]
    if name in ("sin", "cos"):
        edge = [0.0, -0.0, 1e-300, TINY, 1e-9] + [s * k * PI / 4 for k in range(1, 17) for s in (1, -1)]
        edge += [np.nextafter(PI, 0), np.nextafter(PI, 4), 4 * PI, -4 * PI]
        return np.r_[rs.uniform(-4 * PI, 4 * PI, N - N // 10), rs.uniform(-1e-3, 1e-3, N // 10), edge], b
    if name == "exp":
        lo = -745.1332191019411                               # exp(lo) is the smallest subnormal
        edge = [0.0, -0.0, lo, lo - 0.1, -708.3964185322641, -708.4, -1e-300, 1e-300, 709.78, -1.0, 1.0]
        x = np.r_[rs.uniform(lo - 0.5, 0.0, N // 2), rs.uniform(-40.0, 1.0, N // 4), rs.uniform(-746, -700, N // 8),
                  rs.uniform(0.0, 709.78, N // 8), edge]
        return x, b
    if name in ("log", "log10"):
        m, e = rs.uniform(1, 2, N), rs.randint(-1074, 997, N)
        x = np.minimum(np.ldexp(m, e), 1e300)
        near1 = 1.0 + rs.uniform(-1e-3, 1e-3, N // 10) * 10.0 ** rs.uniform(-12, 0, N // 10)
        edge = [1.0, 2.0, 0.5, 10.0, 0.1, 1e-300, 2.2250738585072014e-308, TINY, 1e300, math.sqrt(2), np.nextafter(1, 0),
                np.nextafter(1, 2), 0.125, 1 - 0.125, 0.875]
        return np.r_[x, near1, edge], b
    if name == "pow":
        k = N // 3
        x6 = 10.0 ** rs.uniform(math.log10(15), 50, k)        # Windschitl's x^6
        xl = rs.uniform(1.0, 16.0, k)                          # Lanczos' x^n, n = 0 .. 6
        nl = rs.randint(0, 7, k)
        xm = rs.uniform(0.001, 0.999, N - 2 * k)               # the NFA's tail bound: m^n, m < 1
        nm = np.floor(rs.uniform(1, 700, N - 2 * k) / -np.log(xm)).clip(1, 100000)
        edge_x, edge_n = [15.0, 16.0, 1.0, 2.0, 0.5, 0.0, 10.0], [6, 6, 100000, 6, 1000, 6, 0]
        return np.r_[x6, xl, xm, edge_x], np.r_[np.full(k, 6.0), nl, nm, edge_n]
    if name == "sinh":                                         # Windschitl's sinh(1 / x), x > 15
        x = 10.0 ** rs.uniform(math.log10(15), 12, N)
        return np.r_[1.0 / x, 1.0 / 15.0, 1.0 / np.nextafter(15, 16), 1e-300, TINY], b
    raise KeyError(name)


@pytest.mark.parametrize("name", list(FN))
def test_portable_function_within_its_ulp_bound(pm, name):
    a, b = _args(name)
    got = pm(name, a, b)
    err = _ulps(name, got, a, b)
    worst = int(np.argmax(err))
    assert err.max() <= BOUND[name], "%s(%r%s) = %r: %.3f ulp" % (
        name, a[worst], "" if b is None else ", %r" % b[worst], got[worst], err[worst])


def test_special_values(pm):
    inf, nan = math.inf, math.nan
    s = lambda v: math.copysign(1.0, v)
    y = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 1.0, -1.0, inf, inf, -inf, -inf, 2.0, 2.0, nan, 1.0]
    x = [0.0, 0.0, -0.0, -0.0, -3.0, -3.0, 0.0, -0.0, inf, -inf, inf, -inf, inf, -inf, 1.0, nan]
    want = [0.0, -0.0, PI, -PI, PI, -PI, PI / 2, -PI / 2, PI / 4, 3 * PI / 4, -PI / 4, -3 * PI / 4, 0.0, PI]
    got = pm("atan2", y, x)
    for g, w in zip(got, want):
        assert g == w and s(g) == s(w), (got, want)
    assert np.isnan(got[-2:]).all()
    assert list(pm("exp", [-inf, inf, 800.0, -800.0])) == [0.0, inf, inf, 0.0] and np.isnan(pm("exp", [nan])).all()
    for f in ("log", "log10"):
        g = pm(f, [0.0, -0.0, inf, 1.0])
        assert list(g) == [-inf, -inf, inf, 0.0]
        assert np.isnan(pm(f, [-1.0, nan])).all()
    assert np.isnan(pm("sin", [inf, -inf, nan])).all() and np.isnan(pm("cos", [inf, -inf, nan])).all()
    assert list(pm("pow", [nan, 0.0, 0.0, 2.0], [0.0, 3.0, -1.0, -2.0])) == [1.0, 0.0, inf, 0.25]
    assert list(pm("sinh", [0.0, 800.0, -800.0])) == [0.0, inf, -inf]


def test_outside_the_domain_finite_and_deterministic(pm):
    rs = np.random.RandomState(5)
    x = np.r_[10.0 ** rs.uniform(-300, 300, 2000) * rs.choice([-1, 1], 2000), 1e308, -1e308, 2.0 ** 60]
    for f in ("sin", "cos"):
        g = pm(f, x)
        assert np.isfinite(g).all() and (np.abs(g) <= 1.0).all() and g.tobytes() == pm(f, x).tobytes()
    p = pm("pow", np.abs(x), 0.37)                             # non-integer exponents: exp(y log x)
    assert np.isfinite(p).all() and p.tobytes() == pm("pow", np.abs(x), 0.37).tobytes()
    assert np.isfinite(pm("pow", [1e300, 2.0 ** 1000], [1.0, 1.0])).all()
    sh = pm("sinh", rs.uniform(-700, 700, 1000))
    assert np.isfinite(sh).all()
