"""Time one training step of the dense head (vpk_train_step) at the net's shape, B = 5 (the solver's batch) and B = 32,
or, with --net, one step of the whole net (train.NetTrainer: the conv stack's forward, vpk_train_step_dx, the conv stack's
backward and update).

    python scripts/time_train_step.py [--net] [--batches 5 32] [--steps 30] [--warmup 5] [--out FILE.json]

Each step is timed by a pair of events on the trainer's stream; the result is the median over the steps after the
warm-up steps (code objects, first touch of the buffers).  The bytes are the step's weight traffic, counted from the
shapes: the forward reads every W once, the fused backward-and-update sweep reads and writes every W and its momentum
once, 5 x 4 bytes per parameter = 5.09 GB.  `fraction` is that over the time, relative to 6.29 TB/s, the copy rate an
MI355X sustains (a step at that rate takes 0.81 ms).  Prints one JSON line per batch size.

--net: events around the three parts of every step as well; the FLOP are the conv stack's executed multiply-adds x 2 counted
from the shapes (forward and weight gradient of conv1-5, data gradient of conv2-5: conv1's is never formed)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vanishing_points_2017_amd import train  # noqa: E402

COPY_RATE = 6.29e12        # bytes/s


def time_net(a, torch):
    from vanishing_points_2017_amd import cnn
    rng = np.random.default_rng(0)
    conv = [cnn.Net.LAYER_FLOP[n] for n in train.CONV_LAYERS]
    flop_image = 2 * sum(conv) + sum(conv[1:])
    # random rasters under random-init weights start from a loss in the thousands: a rate at which the steps stay finite
    nt = train.NetTrainer(cnn.synthetic_weights(0), cnn.synthetic_mean(0), params=train.SolverParams(base_lr=1e-7), seed=1)
    results = []
    for b in a.batches:
        rasters = torch.from_numpy(((rng.random((b, 500, 500)) < 0.05) * 255).astype(np.uint8)).to(nt.rt.tdev)
        lab = torch.from_numpy((rng.random((b, 400)) < 0.01).astype(np.float32)).to(nt.rt.tdev)
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            nt.step(rasters, lab)
        nt.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(a.steps)]
        losses = []
        for e in ev:
            x = nt._data(rasters)
            e[0].record(nt.rt.stream)
            top = nt.stack.forward(x)
            e[1].record(nt.rt.stream)
            loss, _, dx = nt.head.step(top.reshape(b, -1), lab, None, want_dx=True)
            e[2].record(nt.rt.stream)
            nt.stack.backward(dx)
            e[3].record(nt.rt.stream)
            losses.append(loss)
        nt.synchronize()
        ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(3)] for e in ev])
        tot = ms.sum(axis=1)
        med = float(np.median(tot))
        res = {"what": "NetTrainer.step", "batch": b, "steps": a.steps, "median_ms": round(med, 3),
               "min_ms": round(float(tot.min()), 3), "max_ms": round(float(tot.max()), 3),
               "median_ms_stack_forward": round(float(np.median(ms[:, 0])), 3),
               "median_ms_head_step_dx": round(float(np.median(ms[:, 1])), 3),
               "median_ms_stack_backward": round(float(np.median(ms[:, 2])), 3),
               "conv_gflop_per_image": round(flop_image / 1e9, 3), "conv_tflop_per_s": round(flop_image * b / (med * 1e-3) / 1e12, 3),
               "loss_first": float(losses[0].cpu()), "loss_last": float(losses[-1].cpu())}
        print(json.dumps(res), flush=True)
        results.append(res)
    nt.close()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", action="store_true", help="time train.NetTrainer.step instead of the head's step")
    ap.add_argument("--batches", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dims", type=int, nargs=4, default=list(train.NET_DIMS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if a.net:
        results = time_net(a, torch)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(results, fh, indent=1)
                fh.write("\n")
        return
    i, h6, h7, o = a.dims
    rng = np.random.default_rng(0)
    blobs = []
    for n, k in ((h6, i), (h7, h6), (o, h7)):
        w = rng.standard_normal((n, k), dtype=np.float32)
        w *= np.float32(np.sqrt(2.0 / k))
        blobs += [w, np.full(n, 0.1, np.float32)]
    params = (i * h6 + h6 * h7 + h7 * o) + (h6 + h7 + o)
    nbytes = 5 * 4 * (i * h6 + h6 * h7 + h7 * o)
    tr = train.Head(a.dims, seed=1)
    tr.load(blobs)
    del blobs
    results = []
    for b in a.batches:
        x = torch.from_numpy(np.maximum(rng.standard_normal((b, i), dtype=np.float32), 0)).to(tr.rt.tdev)
        lab = torch.from_numpy((rng.random((b, o)) < 0.01).astype(np.float32)).to(tr.rt.tdev)
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            tr.step(x, lab)
        tr.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        losses = []
        for e0, e1 in ev:
            e0.record(tr.rt.stream)
            losses.append(tr.step(x, lab)[0])
            e1.record(tr.rt.stream)
        tr.synchronize()
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
        med = float(np.median(ms))
        res = {"what": "vpk_train_step", "dims": list(a.dims), "parameters": params, "batch": b, "steps": a.steps,
               "median_ms": round(med, 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
               "weight_traffic_gb": round(nbytes / 1e9, 4), "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3),
               "fraction_of_copy_rate": round(nbytes / (med * 1e-3) / COPY_RATE, 3),
               "loss_first": float(losses[0].cpu()), "loss_last": float(losses[-1].cpu())}
        print(json.dumps(res), flush=True)
        results.append(res)
    tr.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
