"""Time the result overlays: the 102 scenes of synth's YUD-shape configuration (640 x 480 images, their EM results) rendered
in one batch on the GPU, beside the NumPy reference renderer (tests/overlay_reference.py) on ONE image on the host.

    python scripts/time_overlay.py [--reps 5]

Prints one JSON line: gpu_batch_ms is the wall time of result_plotting.render_em_results_batch for the 102 scenes (median of
--reps after one warm-up; draw lists, uploads, the three launches, the copy back and the synchronise included),
gpu_image_panels_ms the same for the image panels alone, numpy_one_image_ms the float64 reference renderer on the first
scene's image panel (its longdouble pass switched off).  same_pixels: the first scene's image panel equals that renderer's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overlay_reference as R  # noqa: E402
from vanishing_points_2017_amd import calc_horizon, em, result_plotting as P, sphere_mapping, synth  # noqa: E402


def median_ms(f, reps):
    f()                                                    # warm-up: code objects, allocator
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
    sphere_mapping.attach_rasters(scenes)
    results = em.em_batch(scenes)
    rng = np.random.RandomState(7)
    datums, images, horizons = [], [], []
    for sc, res in zip(scenes, results):
        datums.append({'lines': {'lines': sc["l"], 'line_segments': sc["lp"]}, 'sphere_image': sc["sphere_image"],
                       'cnn_prediction': sc["cnn_response"], 'EM_result': res if res["vp"] is not None else None})
        images.append(rng.randint(0, 256, (480, 640, 3)).astype(np.uint8))
        hz = None
        if res["vp"] is not None:
            hp1, hp2 = calc_horizon.calculate_horizon_and_ortho_vp(res, maxbest=20, theta_vmin=np.pi / 10.)[:2]
            hz = ((hp1[0], hp1[1]), (hp2[0], hp2[1]))
        horizons.append(hz)
    lists = [P.line_primitives(d, 640, 480, 4, None) for d in datums]
    out = {"images": len(datums), "lines": int(sum(d['lines']['line_segments'].shape[0] for d in datums)),
           "lines_drawn": int(sum(p[2].size for p in lists)),
           "gpu_batch_ms": median_ms(lambda: P.render_em_results_batch(datums, images, horizons=horizons), a.reps),
           "gpu_image_panels_ms": median_ms(lambda: P.overlay_batch(images, lists, False), a.reps),
           "numpy_one_image_ms": median_ms(lambda: R.render(images[0], *lists[0], extended=False), a.reps)}
    got = P.overlay_batch(images[:1], lists[:1], False)[0]
    out["same_pixels"] = bool(np.array_equal(got, R.render(images[0], *lists[0], extended=False)['rgb']))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
