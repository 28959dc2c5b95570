"""ms per call of the batched EM update -- find_initial_vps_batch, weight_matrix_batch, mstep_batch -- beside the loop over
the single-image entry points (kernels.init_vps, kernels.weight_matrix, kernels.mstep_full) on the same inputs.

Needs the GPU.  Three workloads: the 102 YUD-shape scenes (synth.config_scenes(2)), 256 HLW-shape scenes
(synth.config_scenes(4)) and one image with N = 1000 lines and M = 25 VPs.  The inputs of the weights and the M-step are
what an iteration produces: lsim (sigma = 1) and lweight of the batched line geometry, the initial VPs, the E-step's
p_vl and lvsq at the EM's starting variance.  A batched call is timed with its inputs on the device (it ends in a
synchronise); a loop call is the host-in / host-out call a user of the single entries pays: upload, one workgroup,
synchronise, copy back.  Median wall time of the repetitions, after warm-up of every shape.

Usage:  python scripts/time_emstep.py [--reps 7] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S0 = (np.pi / (1.282 * 20)) * 1e-6            # the EM's starting variance (vp_localisation.py:208)


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def prepare(scenes, vps=None):
    """Device inputs of one workload, and host copies for the loop."""
    import torch
    from vanishing_points_2017_amd import probability_functions as P
    from vanishing_points_2017_amd import sphere_mapping
    from vanishing_points_2017_amd import vp_localisation as V
    from vanishing_points_2017_amd.runtime import get_runtime
    dev = get_runtime(0).tdev
    sphere_mapping.attach_rasters(scenes)
    maps = np.stack([s["cnn_response"] for s in scenes])
    spheres = np.stack([s["sphere_image"] for s in scenes])
    lps = [torch.from_numpy(np.ascontiguousarray(s["lp"], dtype=np.float64)).to(dev) for s in scenes]
    ls = [torch.from_numpy(s["l"] / np.sqrt((s["l"] ** 2).sum(1))[:, None]).to(dev) for s in scenes]
    off = np.concatenate(([0], np.cumsum([s["lp"].shape[0] for s in scenes]))).astype(np.int64)
    pair = (torch.cat(lps), off)
    lsims = V.calc_lsim_batch(pair, sigma=1)
    lscore, langle, llen, off = V.line_geometry_batch(pair, k1=10, k2=4)
    lw = llen * lscore.clamp(0.2, 1)
    if vps is None:
        v0, num = V.find_initial_vps_batch(spheres, maps, 25)
        vs = [v0[b, :k] for b, k in enumerate(num.tolist())]
    else:
        vs = [torch.from_numpy(v).to(dev) for v in vps]
    e = P.calc_probabilities_batch(maps, vs, ls, lps, [v.new_full((len(v),), S0) for v in vs])
    d = {"maps": torch.from_numpy(maps).to(dev), "spheres": torch.from_numpy(spheres).to(dev), "ls": ls, "lw": lw, "off": off,
         "lsims": lsims, "vs": vs, "p_vl": [p.vl for p in e['pdf']], "lvsq": [p.lvsq for p in e['pdf']]}
    d["w"] = V.weight_matrix_batch(d["p_vl"], lw, lsims, bias=1, line_offsets=off)
    cpu = lambda x: [t.cpu().numpy() for t in x]
    lwh = lw.cpu().numpy()
    h = {"maps": maps, "spheres": spheres, "ls": cpu(ls), "lw": [lwh[off[b]:off[b + 1]] for b in range(len(scenes))], "lsims": cpu(lsims),
         "vs": cpu(vs), "p_vl": cpu(d["p_vl"]), "lvsq": [x.T.copy() for x in cpu(d["lvsq"])], "w": cpu(d["w"])}
    return d, h


def time_workload(name, scenes, reps, vps=None):
    from vanishing_points_2017_amd import kernels
    from vanishing_points_2017_amd import vp_localisation as V
    d, h = prepare(scenes, vps)
    B = len(scenes)
    work = [b for b in range(B) if h["vs"][b].shape[0] and h["ls"][b].shape[0]]
    row = {"workload": name, "images": B, "lines": int(d["off"][-1]), "vps": int(sum(v.shape[0] for v in h["vs"]))}
    row["init_batch_ms"] = median_ms(lambda: V.find_initial_vps_batch(d["spheres"], d["maps"], 25), reps, 2)
    row["init_loop_ms"] = median_ms(lambda: [kernels.init_vps(h["maps"][b], h["spheres"][b], 25) for b in range(B)], max(reps // 2, 1), 1)
    row["weights_batch_ms"] = median_ms(lambda: V.weight_matrix_batch(d["p_vl"], d["lw"], d["lsims"], bias=1, line_offsets=d["off"]), reps, 2)
    row["weights_loop_ms"] = median_ms(lambda: [kernels.weight_matrix(h["p_vl"][b], h["lw"][b], h["lsims"][b], 1.0) for b in work],
                                       max(reps // 2, 1), 1)
    row["mstep_batch_ms"] = median_ms(lambda: V.mstep_batch(d["ls"], d["w"], d["lvsq"], d["p_vl"], d["vs"]), reps, 2)
    row["mstep_loop_ms"] = median_ms(lambda: [kernels.mstep_full(h["ls"][b], h["w"][b], h["lvsq"][b], h["p_vl"][b], h["vs"][b]) for b in work],
                                     max(reps // 2, 1), 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from vanishing_points_2017_amd import synth
    print("%-10s %6s %8s %6s | %21s | %21s | %21s" % ("workload", "images", "lines", "VPs", "initial VPs  ms", "weights  ms", "M-step  ms"))
    print("%-10s %6s %8s %6s | %10s %10s | %10s %10s | %10s %10s" % (("", "", "", "") + ("batch", "loop") * 3), flush=True)
    rows = []
    for name, scenes, vps in (("yud-shape", list(synth.config_scenes(2)), None), ("hlw-shape", list(synth.config_scenes(4, count=256)), None),
                              ("n1000-m25", [synth.make_scene(5000, 1000, 3)], [synth.stress_init_vps(5000, m=25)])):
        r = time_workload(name, scenes, a.reps, vps)
        rows.append(r)
        print("%-10s %6d %8d %6d | %10.3f %10.3f | %10.3f %10.3f | %10.3f %10.3f" % (
            r["workload"], r["images"], r["lines"], r["vps"], r["init_batch_ms"], r["init_loop_ms"], r["weights_batch_ms"],
            r["weights_loop_ms"], r["mstep_batch_ms"], r["mstep_loop_ms"]), flush=True)
    print(json.dumps({"emstep_timings": rows}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"emstep_timings": rows}, f, indent=1)


if __name__ == "__main__":
    main()
