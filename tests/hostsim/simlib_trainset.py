"""ctypes access to the TEST-ONLY host build of csrc/trainset_device.hpp (tests/hostsim/sim_trainset.cpp): the per-element
rules of the device-resident training set.  A library of its own, built by hostbuild.py on first use."""
import ctypes

import numpy as np

from . import hostbuild, simlib


def lib():
    return hostbuild.load("trainset")


def _d(a):
    return simlib._p(a, ctypes.c_double)


def draws(seed, iteration, b, count):
    out = np.zeros(count, np.float64)
    lib().sim_trainset_draws(ctypes.c_ulonglong(seed), ctypes.c_ulonglong(iteration), ctypes.c_uint(b), int(count), _d(out))
    return out


def order_keys(seed, epoch, n):
    out = np.zeros(n, np.uint64)
    lib().sim_trainset_order_keys(ctypes.c_ulonglong(seed), ctypes.c_ulonglong(epoch), ctypes.c_longlong(n),
                                  simlib._p(out, ctypes.c_ulonglong))
    return out


def transform(h, l, v):
    """rows of h (n, 6), l (n, 3), v (n, 3) -> (transformed lines, transformed VPs)"""
    h, l, v = (np.ascontiguousarray(a, dtype=np.float64) for a in (h, l, v))
    m, w = np.zeros_like(l), np.zeros_like(v)
    lib().sim_trainset_transform(ctypes.c_longlong(l.shape[0]), _d(h), _d(l), _d(v), _d(m), _d(w))
    return m, w


def cells(v, grid):
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(v.shape[0], np.int32)
    lib().sim_trainset_cells(ctypes.c_longlong(v.shape[0]), _d(v), int(grid[0]), int(grid[1]), simlib._p(out, ctypes.c_int))
    return out


def valid(h):
    return bool(lib().sim_trainset_valid(_d(np.ascontiguousarray(h, dtype=np.float64))))


def slots(offsets):
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    out = np.zeros(int(off[-1]), np.int32)
    lib().sim_trainset_slots(simlib._p(off, ctypes.c_longlong), int(off.shape[0] - 1), ctypes.c_longlong(int(off[-1])),
                             simlib._p(out, ctypes.c_int))
    return out
