"""Time the VP set maintenance outside the EM: the 102 YUD-shape scenes of synth (bench.py's workload), each with the VP
set its own EM run ended with, through calc_vp_line_counts_batch and merge_vps_batch in one launch each, and through 102
single-image calls.

    python scripts/time_vp_set.py [--reps 5] [--measure angle|dotprod|area]

Prints one JSON line: wall times in ms (median of --reps after one warm-up; uploads, the launch and the final synchronise
included; the batch forms' results stay on the device, the single calls copy theirs to the host as they always do).  The
merge runs at thresh = 1e-2, ten times the EM's, so that some of the final VP sets do merge.

--measure: the batch forms are also timed under that distance measure (counts_batch_<measure>_ms, merge_batch_<measure>_ms)
on the same VP sets, next to the "angle" times of the same run; the single-image forms take "angle" only."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vanishing_points_2017_amd import em, synth, probability_functions as P, vp_localisation as V  # noqa: E402


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
    ap.add_argument("--measure", choices=("angle", "dotprod", "area"), default="angle")
    a = ap.parse_args()
    scenes = list(synth.config_scenes(2))
    res = em.em_batch(scenes, want_metric=True)
    keep = [b for b, r in enumerate(res) if r["status"] == 0]
    scenes, res = [scenes[b] for b in keep], [res[b] for b in keep]
    lps = [np.ascontiguousarray(sc["lp"], dtype=np.float64) for sc in scenes]
    ls = [r["l"] for r in res]
    vs, ss, metrics = [r["vp"] for r in res], [r["sigma"] for r in res], [r["decision_metric"] for r in res]
    lscore, _, llen, off = V.line_geometry_batch(lps, k1=10, k2=4, sigma=1)
    lw_all = (llen * lscore.clamp(0.2, 1.0)).cpu().numpy()
    lws = [lw_all[off[b]:off[b + 1]] for b in range(len(lps))]
    lsims = V.calc_lsim_batch(lps, sigma=1)
    lsims_host = [x.cpu().numpy() for x in lsims]
    par = P.pdf_params_batch(np.stack([sc["cnn_response"] for sc in scenes]).astype(np.float32))
    pars = [P.PDFParams(means=P._grid_means(), weights=w, sigma=par.sigma) for w in par.weights.cpu().numpy()]
    thresh = 1e-2
    counts_b = lambda: V.calc_vp_line_counts_batch(vs, lps, ss, metrics, lws, thresh=1.96 ** 2)                     # noqa: E731
    counts_1 = lambda: [V.calc_vp_line_counts(vs[b], ls[b], lps[b], ss[b], metrics[b], lws[b], "angle", thresh=1.96 ** 2)  # noqa: E731
                        for b in range(len(lps))]
    merge_b = lambda: V.merge_vps_batch(vs, ss, ls, thresh, lws, lsims, 1, par, lps)                                 # noqa: E731
    merge_1 = lambda: [V.merge_vps(0, vs[b][None], ss[b], ls[b], thresh, lws[b], lsims_host[b], 1, pars[b], lps[b], None,  # noqa: E731
                                   "angle") for b in range(len(lps))]
    out = {"images": len(lps), "lines": int(sum(x.shape[0] for x in lps)), "vps": int(sum(x.shape[0] for x in vs)),
           "counts_batch_ms": median_ms(counts_b, a.reps), "counts_single_ms": median_ms(counts_1, a.reps),
           "merge_batch_ms": median_ms(merge_b, a.reps), "merge_single_ms": median_ms(merge_1, a.reps)}
    if a.measure != "angle":
        counts_m = lambda: V.calc_vp_line_counts_batch(vs, lps, ss, metrics, lws, a.measure, thresh=1.96 ** 2, ls=ls)   # noqa: E731
        merge_m = lambda: V.merge_vps_batch(vs, ss, ls, thresh, lws, lsims, 1, par, lps, distance_measure=a.measure)   # noqa: E731
        out["counts_batch_%s_ms" % a.measure] = median_ms(counts_m, a.reps)
        out["merge_batch_%s_ms" % a.measure] = median_ms(merge_m, a.reps)
        out["vps_after_merge_%s" % a.measure] = int(merge_m()["num_vp"].sum())
        out["lines_counted_%s" % a.measure] = int(counts_m()[0].sum())
    mb = merge_b()
    out["vps_after_merge"] = int(mb["num_vp"].sum())
    c = counts_b()
    em_counts = np.concatenate([r["counts"] for r in res])
    out["counts_equal_em"] = bool(np.array_equal(c[0].cpu().numpy(), em_counts))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
