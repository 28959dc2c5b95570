"""Line segment detection throughput: the host detector (vpk_lsd_detect) on 1 and on 16 threads against the GPU batch
(vpk_lsd_detect_batch), for B images of 640 x 480 and 640 x 427, rendered scenes (150 strokes, noise sigma 2) and white
noise.  GPU: the wrapper lsd.detect_line_segments_batch (host arrays in and out: upload, detection, download) and the raw
call on device-resident images, timed with a device synchronise.  The per-stage split of the GPU call comes from a
kernel trace of this script (rocprofv3 --kernel-trace --stats -- python scripts/time_lsd.py --gpu-only ...).
Prints one JSON line per image kind.

    python scripts/time_lsd.py [--batch 256] [--host-images 32] [--reps 3] [--gpu-only]
"""
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_frontend import _render  # noqa: E402
from vanishing_points_2017_amd import _lib, lsd  # noqa: E402

args = sys.argv[1:]
B = int(args[args.index("--batch") + 1]) if "--batch" in args else 256
HOST_N = int(args[args.index("--host-images") + 1]) if "--host-images" in args else 32
REPS = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
GPU_ONLY = "--gpu-only" in args
THREADS = 16


def images(kind, h, w, n, distinct=8):
    """n images: `distinct` seeded ones, repeated (the detector's work depends on the content, not on the index)."""
    base = []
    for s in range(distinct):
        rs = np.random.RandomState(100 + s)
        if kind == "scene":
            segs = [tuple(rs.uniform(0, [w, h, w, h])) for _ in range(150)]
            base.append(_render(segs, h, w) + rs.normal(0, 2.0, (h, w)))
        else:
            base.append(rs.uniform(0, 255, (h, w)))
    return [base[k % distinct] for k in range(n)]


def host_rate(imgs, threads):
    t = time.perf_counter()
    if threads == 1:
        for im in imgs:
            lsd.detect_line_segments(im)
    else:
        with ThreadPoolExecutor(threads) as ex:          # ctypes releases the GIL during vpk_lsd_detect
            list(ex.map(lsd.detect_line_segments, imgs))
    return len(imgs) / (time.perf_counter() - t)


def gpu_rates(imgs):
    import torch
    h = _lib.get_handle(0)
    lsd.detect_line_segments_batch(imgs[:2])                         # code objects, workspace
    best_wrap = 0.0
    for _ in range(REPS):
        t = time.perf_counter()
        rows = lsd.detect_line_segments_batch(imgs)
        best_wrap = max(best_wrap, len(imgs) / (time.perf_counter() - t))
    dims = np.array([[im.shape[1], im.shape[0]] for im in imgs], dtype=np.int32)
    offs = np.zeros(len(imgs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([im.size for im in imgs])
    flat = torch.from_numpy(np.concatenate([im.ravel() for im in imgs])).cuda()
    cap = max(r.shape[0] for r in rows)
    out = torch.empty((len(imgs), cap, 7), dtype=torch.float64, device="cuda")
    n = torch.empty(len(imgs), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    best_dev = 0.0
    for _ in range(REPS):
        t = time.perf_counter()
        h.check(h.lib.vpk_lsd_detect_batch(h.h, len(imgs), dims.ctypes.data_as(ctypes.c_void_p),
                                           offs.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(flat.data_ptr()), 0.8,
                                           ctypes.c_void_p(out.data_ptr()), cap, ctypes.c_void_p(n.data_ptr())))
        h.synchronize()
        best_dev = max(best_dev, len(imgs) / (time.perf_counter() - t))
    return best_wrap, best_dev, int(n.cpu().numpy().sum())


for kind in ("scene", "noise"):
    for hh, ww in ((480, 640), (427, 640)):
        imgs = images(kind, hh, ww, B)
        res = {"kind": kind, "size": "%dx%d" % (ww, hh), "batch": B}
        if not GPU_ONLY:
            res["host_1thread_img_s"] = round(host_rate(imgs[:HOST_N], 1), 1)
            res["host_%dthreads_img_s" % THREADS] = round(host_rate(imgs, THREADS), 1)
        wrap, dev, nseg = gpu_rates(imgs)
        res["gpu_with_upload_img_s"] = round(wrap, 1)
        res["gpu_device_resident_img_s"] = round(dev, 1)
        res["segments"] = nseg
        print(json.dumps(res), flush=True)
