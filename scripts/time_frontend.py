"""Image-in front end throughput (frontend.lines_batch_device: vpk_image_prepare_batch -> vpk_lsd_detect_batch ->
vpk_lsd_rows_to_lines -> vpk_sphere_raster) for B decoded RGB images of two shapes: the YUD shape (640 x 480, no resize)
and the HLW shape (2000 x 1333, target_size 800).  Per stage on device-resident buffers (host clock around each call
and a device synchronise, best of --reps), the whole path from host arrays, and two baselines on the same images:
line_detector_batch's chain (Pillow resize + rgb2gray on the host, the GPU detector, lines in numpy) and the host
detector on 16 threads (resize and grey per image on the host too).  Prints one JSON line per shape.  The kernel split
comes from a trace of this script (rocprofv3 --kernel-trace --stats -- python scripts/time_frontend.py --gpu-only ...).

    python scripts/time_frontend.py [--batch 256] [--reps 3] [--gpu-only]
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
from vanishing_points_2017_amd import frontend, lsd  # noqa: E402
from vanishing_points_2017_amd.runtime import get_runtime  # noqa: E402

args = sys.argv[1:]
B = int(args[args.index("--batch") + 1]) if "--batch" in args else 256
REPS = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
GPU_ONLY = "--gpu-only" in args
THREADS = 16


def images(h, w, n, distinct=8):
    """n RGB scenes: `distinct` seeded ones (strokes per channel rendered at up to 640 wide, Pillow-upscaled, noise),
    repeated."""
    from PIL import Image
    base = []
    for s in range(distinct):
        rs = np.random.RandomState(200 + s)
        rh, rw = (h, w) if w <= 640 else (h * 640 // w, 640)
        chans = []
        for c in range(3):
            segs = [tuple(rs.uniform(0, [rw, rh, rw, rh])) for _ in range(60)]
            chans.append(_render(segs, rh, rw) * (0.7 + 0.15 * c))
        im = np.clip(np.stack(chans, 2), 0, 255).astype(np.uint8)
        if (rh, rw) != (h, w):
            im = np.asarray(Image.fromarray(im).resize((w, h), Image.BICUBIC))
        base.append(np.clip(im + rs.normal(0, 2.0, im.shape), 0, 255).astype(np.uint8))
    return [base[k % distinct] for k in range(n)]


def best(fn, sync, reps=REPS):
    fn()
    sync()
    t_best = None
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        sync()
        dt = time.perf_counter() - t
        t_best = dt if t_best is None else min(t_best, dt)
    return t_best


def stages(rt, imgs, target):
    """Seconds per stage on device-resident buffers."""
    torch = rt.torch
    n = len(imgs)
    dims = np.zeros((n, 5), dtype=np.int32)
    for k, im in enumerate(imgs):
        h, w = im.shape[:2]
        ow, oh = (w, h) if target is None else frontend.fit_size(w, h, target)
        dims[k] = (w, h, 3, ow, oh)
    in_off = np.r_[0, np.cumsum([im.size for im in imgs])].astype(np.int64)
    out_off = np.r_[0, np.cumsum(dims[:, 3].astype(np.int64) * dims[:, 4])].astype(np.int64)
    det = np.ascontiguousarray(dims[:, 3:5])
    host = np.concatenate([im.ravel() for im in imgs])
    with rt.on_stream():
        flat = torch.from_numpy(host).to(rt.tdev)
        grey = torch.empty(int(out_off[-1]), dtype=torch.float64, device=rt.tdev)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    t = {}
    t["upload_s"] = best(lambda: flat.copy_(torch.from_numpy(host), non_blocking=False), rt.synchronize)
    t["prepare_s"] = best(lambda: rt.check(rt.lib.vpk_image_prepare_batch(rt.h, n, p(dims), p(in_off), rt.ptr(flat), p(out_off),
                                                                          None, rt.ptr(grey))), rt.synchronize)
    cap = 4096
    with rt.on_stream():
        rows = torch.empty((n, cap, 7), dtype=torch.float64, device=rt.tdev)
        cnt = torch.empty(n, dtype=torch.int32, device=rt.tdev)
    t["detector_s"] = best(lambda: rt.check(rt.lib.vpk_lsd_detect_batch(rt.h, n, p(det), p(out_off), rt.ptr(grey), 0.8, rt.ptr(rows),
                                                                        cap, rt.ptr(cnt))), rt.synchronize)
    counts = cnt.cpu().numpy()
    assert (counts <= cap).all()
    offs = np.r_[0, np.cumsum(counts)].astype(np.int64)
    with rt.on_stream():
        l = torch.empty((int(offs[-1]), 3), dtype=torch.float64, device=rt.tdev)
        lp = torch.empty((int(offs[-1]), 4), dtype=torch.float64, device=rt.tdev)
        sphere = torch.empty((n, 500, 500), dtype=torch.uint8, device=rt.tdev)
    t["rows_to_lines_s"] = best(lambda: rt.check(rt.lib.vpk_lsd_rows_to_lines(rt.h, n, p(det), rt.ptr(rows), cap, p(offs),
                                                                              rt.ptr(lp), rt.ptr(l), None)), rt.synchronize)
    t["raster_s"] = best(lambda: rt.check(rt.lib.vpk_sphere_raster(rt.h, rt.ptr(l), p(offs), n, 500, 0.1, rt.ptr(sphere))),
                         rt.synchronize)
    return t, int(offs[-1])


def host_batch_chain(imgs, target):
    """line_detector_batch without the file decode, then the lines uploaded as em.upload_batch does."""
    import torch
    rgbs = [im if target is None else frontend.resize_to_fit(im, target) for im in imgs]
    greys = [frontend.rgb2gray(im) for im in rgbs]
    raw = lsd.detect_line_segments_batch([frontend._detector_input(g) for g in greys])
    segs = [frontend.detect_lsd_lines(g, detector=lambda image, r=r: r)['segments'] for g, r in zip(greys, raw)]
    lines = [frontend.homogeneous_lines(s) for s in segs]
    torch.from_numpy(np.concatenate(lines)).cuda()
    torch.from_numpy(np.concatenate(segs)).cuda()
    torch.cuda.synchronize()


def host_threads(imgs, target):
    def one(im):
        if target is not None:
            im = frontend.resize_to_fit(im, target)
        return frontend.detect_lsd_lines(frontend.rgb2gray(im))
    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(one, imgs))


rt = get_runtime(0)
for name, (h, w), target in (("yud_640x480", (480, 640), None), ("hlw_2000x1333_to_800", (1333, 2000), 800)):
    imgs = images(h, w, B)
    res = {"shape": name, "batch": B}
    t, nseg = stages(rt, imgs, target)
    for k, v in t.items():
        res[k.replace("_s", "_ms")] = round(v * 1e3, 2)
    res["segments"] = nseg
    dev = sum(v for k, v in t.items() if k != "upload_s")
    res["device_stages_img_s"] = round(B / dev, 1)
    res["detector_only_img_s"] = round(B / t["detector_s"], 1)
    e2e = best(lambda: frontend.lines_batch_device(imgs, target, cnn_input_size=500), rt.synchronize)
    res["lines_batch_device_img_s"] = round(B / e2e, 1)            # host arrays in, device lines + rasters out
    if not GPU_ONLY:
        t0 = time.perf_counter()
        host_batch_chain(imgs, target)
        res["line_detector_batch_chain_img_s"] = round(B / (time.perf_counter() - t0), 1)
        t0 = time.perf_counter()
        host_threads(imgs, target)
        res["host_%dthreads_img_s" % THREADS] = round(B / (time.perf_counter() - t0), 1)
    print(json.dumps(res), flush=True)
