"""Time the batched line geometry on the GPU against what the library offered before it: the 102 line sets of synth's
YUD-shape configuration (100..400 lines each) in one call, and one set of N = 1000 lines.

    python scripts/time_line_geometry.py [--reps 5]

Prints one JSON line per data set with the wall time (median of --reps after one warm-up, upload of the lines and the final
synchronise included; the results stay on the device) of
  batched   vp_localisation.calc_lsim_batch + line_geometry_batch: two launches for the whole set, at the EM's settings
            (sigma = 1, k1 = 10, k2 = 4) so that both columns compute the same numbers
  per_image a Python loop of kernels.pairwise over the images (vpk_pairwise: one workgroup per launch, the distance matrix
            through HBM, the results copied to the host as that wrapper does)
and of the two batched calls alone."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vanishing_points_2017_amd import kernels, synth, vp_localisation as V  # noqa: E402


def median_ms(f, reps):
    f()                                                    # warm-up: code objects, allocator
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()                                                # every call below ends with a synchronise of the library's stream
        times.append(time.perf_counter() - t0)
    return round(float(np.median(times)) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sets = {"yud-shape x102": [sc["lp"] for sc in synth.config_scenes(2)],
            "N=1000 x1": [synth.make_scene(5000, 1000, 8)["lp"]]}
    for name, lps in sets.items():
        lps = [np.ascontiguousarray(lp, dtype=np.float64) for lp in lps]
        sim = lambda: V.calc_lsim_batch(lps, sigma=1)                                  # noqa: E731
        rate = lambda: V.line_geometry_batch(lps, k1=10, k2=4, sigma=1)                # noqa: E731
        out = {"set": name, "images": len(lps), "lines": int(sum(lp.shape[0] for lp in lps)),
               "pairs": int(sum(lp.shape[0] * (lp.shape[0] - 1) // 2 for lp in lps)),
               "batched_ms": median_ms(lambda: (sim(), rate()), a.reps),
               "similarity_ms": median_ms(sim, a.reps), "rating_ms": median_ms(rate, a.reps),
               "per_image_ms": median_ms(lambda: [kernels.pairwise(lp) for lp in lps], a.reps)}
        mats = sim()
        ref = kernels.pairwise(lps[0])
        out["same_bits"] = bool(np.array_equal(mats[0].cpu().numpy(), ref[0]) and
                                np.array_equal(rate()[0][:lps[0].shape[0]].cpu().numpy(), ref[1]))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
