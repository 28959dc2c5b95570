"""Recorded rows of the line segment detector under the portable math policy.

TEST INFRASTRUCTURE.  Loads the g++ build of tests/hostsim/sim_lsd.cpp (the one tests/test_hostsim_lsd.py uses) and stores,
in tests/golden/lsd/lsd_portable.npz, five small images as uint8 grey levels -- so the inputs are the same bytes on every
machine -- and for each the rows of sim_lsd_portable at scales 0.8, 1.0 and 0.5.  The portable policy
(csrc/lsd_portable_math.hpp) is exact arithmetic: the same bits come out whatever libm a machine has, on the host and,
under vpk_lsd_set_math(h, 1), on the GPU.  Recorded from the tree in which csrc/vpk_lsd.cpp was still a detector written
out on its own, which that tree's test_device_source_on_the_host_equals_the_host_detector tied to these functions bit for
bit; the rows pin csrc/lsd_device.hpp to that arithmetic from then on.  Only data is written.

The seeds are chosen so that every image with several strokes gives at least 5 rows at every scale (asserted below);
the 8 x 8 noise gives none, and the 9 x 13 image holds one stroke, whose two edges are all it can give.

Usage:  python oracle/make_lsd_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_frontend import _render  # noqa: E402
from test_hostsim_lsd import build_sim  # noqa: E402

SCALES = (0.8, 1.0, 0.5)
# name -> (seed, strokes, height, width, noise sigma)
STROKES = {"strokes6_48x40": (1, 6, 40, 48, 1.0), "strokes12_96x80": (1, 12, 80, 96, 1.0),
           "strokes20_160x120": (1, 20, 120, 160, 1.5)}


def images():
    out = {"noise_8x8": np.random.RandomState(7).randint(0, 256, (8, 8)), "stroke_9x13": _render([(1, 1, 8, 12)], 13, 9)}
    for name, (seed, n, h, w, noise) in STROKES.items():
        rs = np.random.RandomState(seed)
        segs = [tuple(rs.uniform(0, [w, h, w, h])) for _ in range(n)]
        out[name] = _render(segs, h, w) + rs.normal(0, noise, (h, w))
    return {k: np.clip(np.rint(v), 0, 255).astype(np.uint8) for k, v in out.items()}


def main():
    run = build_sim("sim_lsd_portable")
    out = {}
    for name, img in images().items():
        out["image_" + name] = img
        for scale in SCALES:
            rows = run(img.astype(np.float64), scale)
            out["rows_%s_%g" % (name, scale)] = rows
            print("%-20s scale %g: %d rows" % (name, scale, rows.shape[0]))
            if name in STROKES:
                assert rows.shape[0] >= 5, "choose another seed for " + name
            if name == "noise_8x8":
                assert rows.shape[0] == 0
    path = os.path.join(ROOT, "tests", "golden", "lsd", "lsd_portable.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 64 << 10


if __name__ == "__main__":
    main()
