"""ctypes access to the TEST-ONLY host build of csrc/train_plan.hpp (tests/hostsim/sim_train_plan.cpp): what vpk_train.hip and
vpk_convtrain.hip decide on the host before they launch.  A library of its own, built by hostbuild.py on first use."""
import ctypes

import numpy as np

from . import hostbuild

_I, _F, _U = ctypes.c_int32, ctypes.c_float, ctypes.c_ulonglong
OK, NO_CHAIN, LRN_WIDE = 0, 1, 2                                 # csrc/train_plan.hpp: StackRule
CONV, LRN, POOL = 0, 1, 2                                        # include/vpk.h: VPK_LAYER_*
FWD, DGRAD, WGRAD = 0, 1, 2                                      # csrc/convtrain_device.hpp: GEMM_*
CONSTANTS = ("TRAIN_MAX_B", "FWD_RT", "SWEEP_KT", "SWEEP_MIN_RT", "SWEEP_MAX_RT", "CT_MAX_B", "CT_MAX_LAYERS", "CT_TILE",
             "CT_LRN_PIX", "CT_LRN_MAX_C")


class TrainParams(ctypes.Structure):                             # include/vpk.h: vpk_train_params
    _fields_ = [("base_lr", _F), ("gamma", _F), ("stepsize", ctypes.c_int64), ("momentum", _F), ("weight_decay", _F),
                ("lr_mult_weight", _F), ("decay_mult_weight", _F), ("lr_mult_bias", _F), ("decay_mult_bias", _F),
                ("dropout_ratio", _F)]


class StackLayer(ctypes.Structure):                              # include/vpk.h: vpk_stack_layer
    _fields_ = [(n, _I) for n in ("kind", "out_channels", "kernel", "stride", "pad", "groups", "relu", "local_size")] + \
               [(n, _F) for n in ("alpha", "beta", "k")]


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = hostbuild.load("train_plan")
        _lib.sim_tp_vec.argtypes = [ctypes.c_int, _U, _U, _U, _U]
        _lib.sim_tp_slab_buffer.restype = _U
        _lib.sim_tp_rates.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
        assert constants()["sizes"] == (ctypes.sizeof(TrainParams), ctypes.sizeof(StackLayer))
    return _lib


def constants():
    out = (ctypes.c_int * 12)()
    lib().sim_tp_constants(out)
    return dict(zip(CONSTANTS, out[2:]), sizes=(out[0], out[1]))


def _ints(fn, count, *args):
    out = (ctypes.c_int * count)()
    fn(*(args + (out,)))
    return list(out)


def sweep(n, k):
    """(rows per tile, tiles, column tiles) of the backward's sweep over an n x k layer"""
    return tuple(_ints(lib().sim_tp_sweep, 3, n, k))


def fwd(n, k):
    """(chunks, chunks per slab, slabs, row tiles) of the forward of an n x k layer"""
    return tuple(_ints(lib().sim_tp_fwd, 4, n, k))


def nb(b):
    return lib().sim_tp_nb(b)


def vec(k, ptrs):
    """the float4 rule for rows of k floats behind up to four pointers (integers; 0: a pointer the launch does not use)"""
    p = list(ptrs) + [0] * (4 - len(ptrs))
    return bool(lib().sim_tp_vec(k, *p))


def workspaces(dims, b):
    """bytes of (partial, fpartial, xpartial at a batch of b) for dims = (I, H6, H7, O)"""
    out = (_U * 3)()
    lib().sim_tp_workspaces((ctypes.c_int * 4)(*dims), b, out)
    return tuple(out)


def layer(d):
    """a tests/convtrain_reference.py descriptor as a vpk_stack_layer"""
    if d["kind"] == "conv":
        return StackLayer(kind=CONV, out_channels=d["oc"], kernel=d["k"], stride=d["stride"], pad=d["pad"], groups=d["groups"],
                          relu=int(d["relu"]))
    if d["kind"] == "lrn":
        return StackLayer(kind=LRN, local_size=d["n"], alpha=d["alpha"], beta=d["beta"], k=d["k"])
    return StackLayer(kind=POOL, kernel=d["k"], stride=d["stride"])


def _stack(stack):
    layers = [d if isinstance(d, StackLayer) else layer(d) for d in stack]
    return (StackLayer * max(len(layers), 1))(*layers), len(layers)


def chain(in_shape, stack):
    """(rule, [(OC, OH, OW) of every layer that chained])"""
    arr, n = _stack(stack)
    shapes, count = (ctypes.c_int * (3 * max(n, 1)))(), ctypes.c_int()
    rule = lib().sim_tp_chain(in_shape[0], in_shape[1], in_shape[2], arr, n, shapes, ctypes.byref(count))
    return rule, [tuple(shapes[3 * l:3 * l + 3]) for l in range(count.value)]


def layer_plan(in_shape, stack, l, b):
    """the plan of layer l of a stack that chains, at a batch of b"""
    arr, n = _stack(stack)
    out = (_U * 18)()
    lib().sim_tp_layer(in_shape[0], in_shape[1], in_shape[2], arr, n, l, b, out)
    v = [int(x) for x in out]
    return {"slabs": v[0], "slab_len": v[1], "cols": v[2], "wgrad_bytes": v[3], "grid": {FWD: v[4:7], DGRAD: v[7:10], WGRAD: v[10:13]},
            "lrn_grid": v[13:15], "lrn_lds": v[15], "blob_bytes": v[16], "weights": v[17]}


def slab_buffer(in_shape, stack, b):
    arr, n = _stack(stack)
    return int(lib().sim_tp_slab_buffer(in_shape[0], in_shape[1], in_shape[2], arr, n, b))


def kept(events):
    """the kept blobs after `events` (0: a forward begins to launch, B > 0: it is done, -1: a backward is done):
    (backward allowed, read allowed, gradient read allowed, the backward's batch, the read's batch)"""
    ev = (ctypes.c_int * max(len(events), 1))(*events)
    out = _ints(lib().sim_tp_kept, 5, ev, len(events))
    return bool(out[0]), bool(out[1]), bool(out[2]), out[3], out[4]


def params(**kw):
    """vpk_train_default_params (csrc/vpk_train.hip), written out"""
    p = TrainParams(base_lr=1e-4, gamma=0.1, stepsize=200000, momentum=0.9, weight_decay=5e-4, lr_mult_weight=1.0,
                    decay_mult_weight=1.0, lr_mult_bias=2.0, decay_mult_bias=0.0, dropout_ratio=0.5)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def rates(p, iteration):
    """(lr_w, dec_w, lr_b, dec_b, mu) as float32"""
    out = np.zeros(5, np.float32)
    lib().sim_tp_rates(ctypes.addressof(p), int(iteration), out.ctypes.data)
    return out


def params_ok(p, head):
    return bool(lib().sim_tp_params_ok(ctypes.byref(p), int(head)))
