"""ctypes access to the TEST-ONLY host build of csrc/convtrain_device.hpp (tests/hostsim/sim_convtrain.cpp): the per-element
rules of the conv stack's training step.  A library of its own, built by hostbuild.py on first use."""
import ctypes

import numpy as np

from . import hostbuild, simlib

FWD, DGRAD, WGRAD = 0, 1, 2
TILE, CHUNK, TARGET = 64, 16, 1024          # csrc/train_plan.hpp: CT_TILE, CT_CHUNK, CT_TARGET_BLOCKS


def lib():
    return hostbuild.load("convtrain")


def conv_out_size(size, k, stride, pad):
    return lib().sim_ct_conv_out_size(int(size), int(k), int(stride), int(pad))


def pool_out_size(size, k, stride):
    return lib().sim_ct_pool_out_size(int(size), int(k), int(stride))


def pool_window(o, k, stride, size):
    lo, hi = ctypes.c_int(), ctypes.c_int()
    lib().sim_ct_pool_window(int(o), int(k), int(stride), int(size), ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def pool_windows_of(i, k, stride, out):
    lo, hi = ctypes.c_int(), ctypes.c_int()
    lib().sim_ct_pool_windows_of(int(i), int(k), int(stride), int(out), ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def pool_forward(x, k, stride):
    """x (planes, H, W) float32 -> (y, idx)"""
    F, I, P = ctypes.c_float, ctypes.c_int32, simlib._p
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, h, w = x.shape
    oh, ow = pool_out_size(h, k, stride), pool_out_size(w, k, stride)
    y, idx = np.zeros((n, oh, ow), np.float32), np.zeros((n, oh, ow), np.int32)
    lib().sim_ct_pool_forward(P(x, F), n, h, w, int(k), int(stride), P(y, F), P(idx, I))
    return y, idx


def pool_backward(dy, idx, hw, k, stride):
    F, I, P = ctypes.c_float, ctypes.c_int32, simlib._p
    dy, idx = np.ascontiguousarray(dy, dtype=np.float32), np.ascontiguousarray(idx, dtype=np.int32)
    dx = np.zeros((dy.shape[0],) + tuple(hw), np.float32)
    lib().sim_ct_pool_backward(P(dy, F), P(idx, I), dy.shape[0], int(hw[0]), int(hw[1]), int(k), int(stride), P(dx, F))
    return dx


def lrn_forward(x, n, alpha, beta, k):
    """one channel column x (C,) -> (s, y)"""
    F, P = ctypes.c_float, simlib._p
    x = np.ascontiguousarray(x, dtype=np.float32)
    s, y = np.zeros_like(x), np.zeros_like(x)
    lib().sim_ct_lrn_forward(P(x, F), x.size, int(n), F(alpha), F(beta), F(k), P(s, F), P(y, F))
    return s, y


def lrn_backward(x, y, s, dy, n, alpha, beta):
    F, P = ctypes.c_float, simlib._p
    x, y, s, dy = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, y, s, dy))
    ratio, dx = np.zeros_like(x), np.zeros_like(x)
    lib().sim_ct_lrn_backward(P(x, F), P(y, F), P(s, F), P(dy, F), x.size, int(n), F(alpha), F(beta), P(ratio, F), P(dx, F))
    return dx


def _geom(x_shape, d):
    b, c, h, w = x_shape
    oh, ow = conv_out_size(h, d["k"], d["stride"], d["pad"]), conv_out_size(w, d["k"], d["stride"], d["pad"])
    return np.array([c, h, w, d["oc"], d["k"], d["stride"], d["pad"], d["groups"], int(bool(d["relu"])), oh, ow, b], np.int32), oh, ow


def wgrad_slabs(x_shape, d):
    g, _, _ = _geom(x_shape, d)
    slabs, length = ctypes.c_int(), ctypes.c_int()
    lib().sim_ct_wgrad_slabs(simlib._p(g, ctypes.c_int32), TILE, CHUNK, TARGET, ctypes.byref(slabs), ctypes.byref(length))
    return slabs.value, length.value


def _gemm(mode, g, x, w, bias, top, dy, out, slabs, slab_len):
    F, P = ctypes.c_float, simlib._p
    lib().sim_ct_gemm(mode, P(g, ctypes.c_int32), P(x, F), P(w, F), P(bias, F), P(top, F), P(dy, F), P(out, F), int(slabs),
                      int(slab_len))


def conv_forward(x, w, bias, d):
    x, w, bias = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, w, bias))
    g, oh, ow = _geom(x.shape, d)
    out = np.full((x.shape[0], d["oc"], oh, ow), np.nan, np.float32)
    _gemm(FWD, g, x, w, bias, None, None, out, 1, w[0].size)
    return out


def conv_dgrad(x_shape, w, top, dy, d):
    w, top, dy = (np.ascontiguousarray(a, dtype=np.float32) for a in (w, top, dy))
    g, _, _ = _geom(x_shape, d)
    out = np.full(x_shape, np.nan, np.float32)
    _gemm(DGRAD, g, None, w, None, top, dy, out, 1, (d["oc"] // d["groups"]) * d["k"] * d["k"])
    return out


def conv_wgrad(x, top, dy, d):
    """(dW, db): the slabs of the kernel's own split, added in slab order in float32"""
    x, top, dy = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, top, dy))
    g, _, _ = _geom(x.shape, d)
    slabs, slab_len = wgrad_slabs(x.shape, d)
    icg = x.shape[1] // d["groups"]
    cols = icg * d["k"] * d["k"] + 1
    part = np.full((slabs, d["oc"], cols), np.nan, np.float32)
    _gemm(WGRAD, g, x, None, None, top, dy, part, slabs, slab_len)
    acc = np.zeros((d["oc"], cols), np.float32)
    for t in range(slabs):
        acc = (acc + part[t]).astype(np.float32)
    return acc[:, :-1].reshape(d["oc"], icg, d["k"], d["k"]), acc[:, -1], slabs
