"""Time the data path of a solver iteration beside its step: train.TrainSet.batch (vpk_trainset_batch + vpk_sphere_raster)
and train.NetTrainer.step at the net's geometry, B = 5 (the prototxt's batch) and B = 32, on the synthetic YUD-shape set
(synth config 2: 102 images of 100-400 lines, 3 VPs), augmented.

    python scripts/time_train_solver.py [--batches 5 32] [--steps 30] [--warmup 5] [--out FILE.json]

The set lives on the trainer's runtime, so both halves run on one stream and three events on it bracket them: before the
batch, between batch and step, after the step.  The result is the median and the range over the steps after the warm-up
(code objects, first touch of the buffers, the raster's workspace).  `data_share` is the batch's part of the two medians'
sum.  `wall_ms_per_iteration` is the host's clock over the whole timed loop divided by its iterations: what a solver
iteration costs with the host's part (offsets, draws, launches, the raster's offset upload) included.
Prints one JSON line per batch size."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vanishing_points_2017_amd import cnn, synth, train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    # random-init weights start from a loss in the thousands: a rate at which the steps stay finite (time_train_step.py)
    nt = train.NetTrainer(cnn.synthetic_weights(0), cnn.synthetic_mean(0), params=train.SolverParams(base_lr=1e-7), seed=1)
    scenes = list(synth.config_scenes(2))
    ts = train.TrainSet.from_scenes(scenes, size=500, runtime=nt.rt)
    aug = train.Augment(0.3, 1.25, 0.1, 0.5)
    lines = np.diff(ts.line_offsets)
    results = []
    for b in a.batches:
        nt.iteration = 0
        for t in range(a.warmup):
            nt.step(*ts.batch(t, b, seed=1, augment=aug, shuffle=True))
        nt.synchronize()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.steps)]
        losses = []
        t0 = time.perf_counter()
        for k, e in enumerate(ev):
            e[0].record(nt.rt.stream)
            rasters, labels = ts.batch(a.warmup + k, b, seed=1, augment=aug, shuffle=True)
            e[1].record(nt.rt.stream)
            losses.append(nt.step(rasters, labels)[0])
            e[2].record(nt.rt.stream)
        nt.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / a.steps
        ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(2)] for e in ev])
        med = np.median(ms, axis=0)
        res = {"what": "TrainSet.batch + NetTrainer.step", "batch": b, "steps": a.steps, "set_images": len(ts),
               "set_lines_mean": round(float(lines.mean()), 1),
               "batch_median_ms": round(float(med[0]), 3), "batch_min_ms": round(float(ms[:, 0].min()), 3),
               "batch_max_ms": round(float(ms[:, 0].max()), 3),
               "step_median_ms": round(float(med[1]), 3), "step_min_ms": round(float(ms[:, 1].min()), 3),
               "step_max_ms": round(float(ms[:, 1].max()), 3),
               "data_share": round(float(med[0] / (med[0] + med[1])), 4), "wall_ms_per_iteration": round(wall, 3),
               "loss_first": float(losses[0].cpu()), "loss_last": float(losses[-1].cpu())}
        print(json.dumps(res), flush=True)
        results.append(res)
    nt.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
