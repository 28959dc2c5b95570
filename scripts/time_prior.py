"""Time probability_functions.pdf_grid_batch on the GPU: 102 response maps (the YUD test set's size) at N = 50 (the
reference's default mesh) and N = 500 (the sphere raster's resolution).

    python scripts/time_prior.py [--maps 102] [--reps 5]

Prints one JSON line per N: wall time of the whole call (upload of the maps and the mesh, vpk_prior_params,
vpk_mixture_pdf, synchronise; the density stays on the device), median and spread over the repetitions after one
warm-up call, and the time per point.  The reference's CPU loop takes about 1.2 ms per point."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vanishing_points_2017_amd import probability_functions as prob  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=102)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50, 500])
    a = ap.parse_args()
    rng = np.random.RandomState(7)
    logits = rng.standard_normal((a.maps, 400)) * 3.0
    maps = np.exp(logits - logits.max(axis=1, keepdims=True))
    maps = (maps / maps.sum(axis=1, keepdims=True)).astype(np.float32).reshape(a.maps, 20, 20)   # softmax outputs, as the CNN's
    for n in a.sizes:
        out = prob.pdf_grid_batch(maps, N=n)               # warm-up: code objects, allocator
        assert tuple(out["p"].shape) == (a.maps, n, n)
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = prob.pdf_grid_batch(maps, N=n)           # ends with a synchronise of the library's stream
            times.append(time.perf_counter() - t0)
        points = a.maps * n * n
        med = float(np.median(times))
        print(json.dumps({"maps": a.maps, "N": n, "points": points, "median_ms": round(med * 1e3, 3),
                          "min_ms": round(min(times) * 1e3, 3), "max_ms": round(max(times) * 1e3, 3),
                          "ns_per_point": round(med / points * 1e9, 3),
                          "checksum": float(out["p"].sum().cpu())}), flush=True)


if __name__ == "__main__":
    main()
