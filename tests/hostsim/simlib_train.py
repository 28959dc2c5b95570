"""ctypes access to the TEST-ONLY host build of csrc/train_device.hpp (tests/hostsim/sim_train.cpp): the per-element
functions of the dense head's training step.  A library of its own, built by hostbuild.py on first use."""
import ctypes

import numpy as np

from . import hostbuild, simlib

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = hostbuild.load("train")
        _lib.sim_train_learning_rate.restype = ctypes.c_float
        _lib.sim_train_learning_rate.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_longlong, ctypes.c_longlong]
    return _lib


def loss(z, t, inv_b):
    """(loss term, sigmoid, gradient) per element, float32"""
    F, P = ctypes.c_float, simlib._p
    z, t = np.ascontiguousarray(z, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32)
    out = [np.zeros(z.shape, np.float32) for _ in range(3)]
    lib().sim_train_loss(ctypes.c_longlong(z.size), P(z, F), P(t, F), F(inv_b), *[P(o, F) for o in out])
    return out


def learning_rate(base_lr, gamma, stepsize, iteration):
    return np.float32(lib().sim_train_learning_rate(base_lr, gamma, int(stepsize), int(iteration)))


def sgd_update(w, v, g, lr_local, decay_local, mu):
    """(w', v') of Caffe's update, float32"""
    F, P = ctypes.c_float, simlib._p
    w, v = np.array(w, dtype=np.float32), np.array(v, dtype=np.float32)
    g = np.ascontiguousarray(g, dtype=np.float32)
    lib().sim_train_sgd_update(ctypes.c_longlong(w.size), P(w, F), P(v, F), P(g, F), F(lr_local), F(decay_local), F(mu))
    return w, v


def mask(seed, iteration, layer, batch, width, dropout_ratio=0.5):
    """the (batch, width) uint8 keep mask of drop6 (layer 6) or drop7 (layer 7)"""
    out = np.zeros((batch, width), np.uint8)
    lib().sim_train_mask(ctypes.c_ulonglong(seed), ctypes.c_ulonglong(iteration), ctypes.c_uint(layer), int(batch), int(width),
                         ctypes.c_float(dropout_ratio), simlib._p(out, ctypes.c_ubyte))
    return out
