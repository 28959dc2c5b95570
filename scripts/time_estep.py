"""Time the E-step outside the EM: the 102 YUD-shape scenes of synth (bench.py's workload), each with the VP set its own EM
run ended with, through one calc_probabilities_batch call per distance measure, and through 102 kernels.estep calls (the
single-image, "angle"-only hook that was the only way to these numbers before); and one 250-line image against 4096 VP
hypotheses through calc_lvsq_batch (lvsq only: the launch splits the VP range).

    python scripts/time_estep.py [--reps 5]

Prints one JSON line: wall times in ms (median of --reps after one warm-up; uploads, the launches and the final
synchronise included; the batch forms' results stay on the device, kernels.estep copies its to the host as it always
does)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vanishing_points_2017_amd import em, kernels, synth, probability_functions as P  # noqa: E402


def median_ms(f, reps):
    f()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        times.append(time.perf_counter() - t0)
    return round(float(np.median(times)) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    scenes = list(synth.config_scenes(2))
    res = em.em_batch(scenes)
    keep = [b for b, r in enumerate(res) if r["status"] == 0]
    scenes, res = [scenes[b] for b in keep], [res[b] for b in keep]
    lps = [np.ascontiguousarray(sc["lp"], dtype=np.float64) for sc in scenes]
    ls = [np.ascontiguousarray(r["l"], dtype=np.float64) for r in res]
    vs, ss = [r["vp"] for r in res], [r["sigma"] for r in res]
    maps = np.stack([sc["cnn_response"] for sc in scenes]).astype(np.float32)
    out = {"images": len(lps), "lines": int(sum(x.shape[0] for x in lps)), "vps": int(sum(x.shape[0] for x in vs))}
    for measure in ("angle", "dotprod", "area"):
        out["batch_%s_ms" % measure] = median_ms(
            lambda: P.calc_probabilities_batch(maps, vs, ls, lps, ss, distance_measure=measure), a.reps)
    out["single_angle_ms"] = median_ms(
        lambda: [kernels.estep(lps[b], maps[b], vs[b], ss[b]) for b in range(len(lps))], a.reps)
    rs = np.random.RandomState(0)
    big = max(lps, key=len)
    big = np.tile(big, (250 // big.shape[0] + 1, 1))[:250]
    hyp = rs.randn(4096, 3)
    hyp[:, 2] = np.abs(hyp[:, 2]) + 0.05
    hyp /= np.sqrt((hyp * hyp).sum(1))[:, None]
    out["lvsq_250x4096_ms"] = median_ms(lambda: P.calc_lvsq_batch([hyp], None, [big], distance_measure="angle"), a.reps)
    one = P.calc_probabilities_batch(maps[:1], vs[:1], ls[:1], lps[:1], ss[:1])["pdf"][0]
    _, lvsq, _, _, _ = kernels.estep(lps[0], maps[0], vs[0], ss[0])
    out["lvsq_equal_em"] = bool(np.array_equal(one.lvsq.cpu().numpy(), lvsq, equal_nan=True))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
