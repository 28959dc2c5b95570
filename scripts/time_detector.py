"""Time detector.Detector.detect_device against the three-call flow of example.run_folder on the same images.

    python scripts/time_detector.py [--reps 5] [--batches 16 256]

The images are drawn 640 x 480 scenes (synth.make_scene, 60 lines each, strokes drawn with Pillow and blurred), written as
PNG files so that both paths decode the same bytes before the clock starts.  A random-init net stands in for the trained
one; both paths run it on the same rasters.  Prints one JSON line per batch size with the median of --reps runs, after one
warm-up, of
  detector_ms        Detector.detect_device (cnn_input_size 500, target_size 640, maxbest 20), wall time with the final
                     synchronise, and per stage from events recorded on the runtime's stream as each stage is enqueued
                     (frontend, cnn, em, horizon, pixels; the front end ends with a synchronise of its own)
  run_folder_ms      the flow of example.run_folder with the GPU front end (--lsd gpu-frontend): create_data_pickles,
                     run_cnn, run_em, then the horizon and its pixels per image -- wall time per call, pickles included,
                     since the pickles are how its calls hand their results on
Decoding the files is outside both clocks."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vanishing_points_2017_amd import calc_horizon, cnn, evaluation, frontend, synth  # noqa: E402
from vanishing_points_2017_amd.detector import Detector  # noqa: E402

W, H = 640, 480
STAGES = ("frontend", "cnn", "em", "horizon", "pixels")


def draw_scene(seed):
    from PIL import Image, ImageDraw, ImageFilter
    s = synth.make_scene(seed, 60, 3, aspect_h=float(H) / W)["lp"]
    px = np.stack([s[:, 0] * W / 2 + W / 2, -s[:, 1] * W / 2 + H / 2, s[:, 2] * W / 2 + W / 2, -s[:, 3] * W / 2 + H / 2], axis=1)
    im = Image.new("RGB", (W, H), (220, 215, 205))
    d = ImageDraw.Draw(im)
    for x1, y1, x2, y2 in px:
        d.line([(x1, y1), (x2, y2)], fill=(40, 45, 50), width=3)
    return im.filter(ImageFilter.GaussianBlur(0.8))


def time_detector(det, images, reps):
    import torch
    rows = []
    for r in range(reps + 1):
        ev = {}

        def on_stage(rt, name):
            ev[name] = torch.cuda.Event(enable_timing=True)
            ev[name].record(rt.stream)

        t0 = time.perf_counter()
        det.detect_device(images, on_stage=on_stage)              # ends with a synchronise
        wall = (time.perf_counter() - t0) * 1e3
        names = ("start",) + STAGES
        rows.append([wall] + [ev[a].elapsed_time(ev[b]) for a, b in zip(names[:-1], names[1:])])
    med = np.median(np.array(rows[1:]), axis=0)                   # the first run is the warm-up
    out = {"detector_ms": round(float(med[0]), 3)}
    out.update({"detector_%s_ms" % n: round(float(v), 3) for n, v in zip(STAGES, med[1:])})
    return out


def run_folder_flow(source, dest, net):
    """example.run_folder's calls (example.py:30-76 of the reference) with the GPU front end; wall time of each."""
    t = [time.perf_counter()]
    dataset = evaluation.get_data_list(source, dest, 'default_net', "", "0", distance_measure='angle', use_weights=True,
                                       do_split=True, do_merge=True, update=True)
    evaluation.create_data_pickles(dataset, update=True, cnn_input_size=500, target_size=640, frontend_device=0)
    t.append(time.perf_counter())
    evaluation.run_cnn(dataset, None, None, None, gpu=0, net=net)
    t.append(time.perf_counter())
    evaluation.run_em(dataset)
    t.append(time.perf_counter())
    for data_file in dataset['pickle_files']:
        datum = evaluation._load_pickle(data_file)
        res = datum['EM_result']
        if res is None or res['vp'] is None:
            continue
        height, width = datum['lines']['image_shape'][:2]
        hp1, hp2 = calc_horizon.calculate_horizon_and_ortho_vp(res, maxbest=20, theta_vmin=np.pi / 10.)[:2]
        scale = max(width, height)
        for hp in (hp1, hp2):
            hp[0] = hp[0] * scale / 2.0 + width / 2.0
            hp[1] = -hp[1] * scale / 2.0 + height / 2.0
    t.append(time.perf_counter())
    return [(b - a) * 1e3 for a, b in zip(t[:-1], t[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256])
    a = ap.parse_args()
    net = cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0))
    det = Detector(net, target_size=640, cnn_input_size=500, maxbest=20)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "images")
        os.makedirs(src)
        for k in range(max(a.batches)):
            draw_scene(7000 + k).save(os.path.join(src, "scene_%04d.png" % k))
        files = sorted(os.listdir(src))
        for n in a.batches:
            sub = os.path.join(tmp, "images_%d" % n)
            os.makedirs(sub)
            for f in files[:n]:
                os.symlink(os.path.join(src, f), os.path.join(sub, f))
            images = [frontend.imread(os.path.join(sub, f)) for f in files[:n]]
            out = {"images": n, "size": "%dx%d" % (W, H), "reps": a.reps}
            out.update(time_detector(det, images, a.reps))
            d = det.detect_device(images)
            out["lines"] = int(d["offsets"][-1])
            out["images_with_vps"] = int((d["status"] == 0).sum().item())
            rows = []
            try:
                for r in range(a.reps + 1):
                    with contextlib.redirect_stdout(io.StringIO()):
                        rows.append(run_folder_flow(sub, os.path.join(tmp, "dest_%d_%d" % (n, r)), net))
            except Exception as e:          # run_em raises mid-batch for an image without an initial VP; the detector does not
                out["run_folder_error"] = "%s: %s" % (type(e).__name__, e)
                print(json.dumps(out), flush=True)
                continue
            med = np.median(np.array(rows[1:]), axis=0)
            out["run_folder_ms"] = round(float(np.median(np.array(rows[1:]).sum(axis=1))), 3)
            out.update({"run_folder_%s_ms" % k: round(float(v), 3)
                        for k, v in zip(("create_data_pickles", "run_cnn", "run_em", "horizon"), med)})
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
