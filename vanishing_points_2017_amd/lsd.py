"""`lsd.detect_line_segments(image)` -- the call the reference makes into its un-vendored `lsdpython` submodule
(evaluation.py:7,238; .gitmodules:1-3).  Backed by the detector of libvpk.so (csrc/lsd_device.hpp: the published LSD
algorithm with its default parameters; parity with the absent original is unpinned), run on the host for one image
(vpk_lsd_detect, csrc/vpk_lsd.cpp).  `detect_line_segments_batch(images)` runs the same source for a list of images in one
GPU call (vpk_lsd_detect_batch, csrc/vpk_lsd_gpu.hip); the host call stays the default everywhere."""
import ctypes

import numpy as np

from . import _lib
from .ragged import offsets_of

_BATCH_CAP = 4096          # rows per image of detect_line_segments_batch's first call


def detect_line_segments(image, scale=0.8):
    """image: 2-D array of grey levels 0..255 -> (N, 7) float64: x1, y1, x2, y2, width, p, -log10(NFA)
    in pixel coordinates (x = column, y = row)."""
    img = np.ascontiguousarray(image, dtype=np.float64)
    if img.ndim != 2:
        raise ValueError("detect_line_segments expects a 2-D grey-level image")
    lib = _lib.load()
    h, w = img.shape
    cap = 4096
    while True:
        out = np.zeros((cap, 7), dtype=np.float64)
        n = ctypes.c_int(0)
        rc = lib.vpk_lsd_detect(img.ctypes.data_as(ctypes.c_void_p), int(w), int(h), float(scale),
                                out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n))
        if rc != 0:
            raise _lib.VpkError("vpk_lsd_detect failed with %d (image %d x %d)" % (rc, w, h))
        if n.value <= cap:
            return out[:n.value].copy()
        cap = n.value


def detect_line_segments_batch(images, scale=0.8, device=0):
    """images: list of 2-D arrays of grey levels 0..255 -> list of (N_i, 7) float64 arrays, the rows
    detect_line_segments gives for each image (up to the last bits of the coordinates and of -log10(NFA):
    include/vpk.h, vpk_lsd_detect_batch), detected on GPU `device` in one call.  No CPU fallback."""
    imgs = [np.ascontiguousarray(im, dtype=np.float64) for im in images]
    for im in imgs:
        if im.ndim != 2:
            raise ValueError("detect_line_segments_batch expects 2-D grey-level images")
    if not imgs:
        return []
    import torch
    h = _lib.get_handle(device)
    dev = torch.device("cuda", int(device))
    dims = np.array([[im.shape[1], im.shape[0]] for im in imgs], dtype=np.int32)
    offsets = offsets_of([im.size for im in imgs])
    flat = torch.from_numpy(np.concatenate([im.ravel() for im in imgs])).to(dev)
    torch.cuda.synchronize(dev)               # the upload runs on torch's stream, the detector on the handle's

    def run(idx, cap):
        sel = np.asarray(idx)
        d = np.ascontiguousarray(dims[sel])
        offs = offsets_of(d[:, 0].astype(np.int64) * d[:, 1])
        sub = flat if len(idx) == len(imgs) else torch.cat([flat[offsets[i]:offsets[i + 1]] for i in idx])
        out = torch.empty((len(idx), cap, 7), dtype=torch.float64, device=dev)
        n = torch.zeros(len(idx), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        h.check(h.lib.vpk_lsd_detect_batch(h.h, len(idx), d.ctypes.data_as(ctypes.c_void_p),
                                           offs.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(sub.data_ptr()),
                                           float(scale), ctypes.c_void_p(out.data_ptr()), cap, ctypes.c_void_p(n.data_ptr())))
        h.synchronize()
        return out.cpu().numpy(), n.cpu().numpy()

    res = [None] * len(imgs)
    todo, cap = list(range(len(imgs))), _BATCH_CAP
    while todo:
        out, n = run(todo, cap)
        again = []
        for k, i in enumerate(todo):
            if n[k] <= cap:
                res[i] = out[k, :n[k]].copy()
            else:
                again.append(i)
        cap = int(n.max()) if again else cap
        todo = again
    return res
