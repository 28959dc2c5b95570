"""The REFERENCE's coordinate_conversion for a set of indices, angles and points -> tests/golden/plotting/coconv.npz.

TEST INFRASTRUCTURE, build container only (needs the reference tree; see oracle/ref_shim.py).  Runs the reference's own
index_to_angle, angle_to_index, angle_to_point and point_to_angle (coordinate_conversion.py:4-61), one call per row, and
writes numeric arrays only.

Usage:  python scripts/make_plotting_golden.py

Shapes: (20, 20), (500, 500), (250, 500).
Angles (the same 1009 for every shape): (0, 0) and the eight combinations of 0 and +-pi/2, then 1000 seeded uniform angles
of the square.  For angle_to_point 12 more whose alpha lies beyond +-pi/2, where point[2] < 0 and :48 flips the sign.  (No
float64 angle has a cosine of exactly 0, so point[2] == 0 cannot come out of angle_to_point; at alpha = +-pi/2 it is
+-6.1e-17 cos(beta).)
Indices (per shape): the four corner cells, the cells next to the centre, 200 seeded whole indices and 200 fractional.
Points for point_to_angle: 200 seeded unit vectors (half of them with point[2] < 0), (1, 0, 0), (-1, 0, 0), (0.6, 0.8, 0)
and (0, 0, 0) with point[2] == 0, (0, 1, 0) and (0, -1, 0) where :56 divides by cos(+-pi/2) = 6.1e-17, and two points
whose quotient leaves [-1, 1] and is clamped (:57-58).  sign0 is np.sign(0.0) as the container's NumPy returns it.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from ref_shim import load_reference  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = [(20, 20), (500, 500), (250, 500)]


def main():
    warnings.filterwarnings("ignore")
    np.seterr(all="ignore")
    cc = load_reference()["coordinate_conversion"]
    rng = np.random.RandomState(20170328)
    h = np.pi / 2

    angles = np.concatenate([[[a, b] for a in (0.0, -h, h) for b in (0.0, -h, h)], rng.uniform(-h, h, (1000, 2))])
    assert angles.shape == (1009, 2) and tuple(angles[0]) == (0.0, 0.0)
    a2i = np.stack([np.stack([cc.angle_to_index(a, s) for a in angles]) for s in SHAPES])

    indices, i2a = [], []
    for (m, n) in SHAPES:
        idx = np.concatenate([
            [[0, 0], [0, n - 1], [m - 1, 0], [m - 1, n - 1], [m // 2, n // 2], [m // 2 - 1, n // 2 - 1]],
            np.stack([rng.randint(0, m, 200), rng.randint(0, n, 200)], axis=1),
            np.stack([rng.uniform(-1, m, 200), rng.uniform(-1, n, 200)], axis=1)]).astype(np.float64)
        indices.append(idx)
        i2a.append(np.stack([cc.index_to_angle(i, (m, n)) for i in idx]))
    indices, i2a = np.stack(indices), np.stack(i2a)

    beyond = np.stack([np.concatenate([rng.uniform(h + 0.01, np.pi, 6), rng.uniform(-np.pi, -h - 0.01, 6)]),
                       rng.uniform(-h, h, 12)], axis=1)
    p_angles = np.concatenate([angles, beyond])
    a2p = np.stack([cc.angle_to_point(a) for a in p_angles])
    assert (np.cos(beyond[:, 0]) * np.cos(beyond[:, 1]) < 0).all() and (a2p[-12:, 2] > 0).all()

    pts = rng.standard_normal((200, 3))
    pts /= np.linalg.norm(pts, axis=1)[:, None]
    pts[:100, 2] = -np.abs(pts[:100, 2])
    pts = np.concatenate([pts, [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0],
                                [0.0, -1.0, 0.0], [0.9, 0.6, 0.1], [-0.9, 0.6, 0.1]]])
    p2a = np.stack([cc.point_to_angle(p) for p in pts])

    os.makedirs(os.path.join(GOLDEN, "plotting"), exist_ok=True)
    out = os.path.join(GOLDEN, "plotting", "coconv.npz")
    np.savez_compressed(out, shapes=np.array(SHAPES, dtype=np.int64), angles=angles, angle_to_index=a2i, indices=indices,
                        index_to_angle=i2a, point_angles=p_angles, angle_to_point=a2p, points=pts, point_to_angle=p2a,
                        sign0=np.float64(np.sign(0.0)))
    print("%s: %d bytes; NaN angles from points: %d" % (out, os.path.getsize(out), int(np.isnan(p2a).any(axis=1).sum())))


if __name__ == "__main__":
    main()
