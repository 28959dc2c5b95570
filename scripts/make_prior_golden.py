"""The REFERENCE's prior density for a few response maps -> tests/golden/prior/prior_pdf.npz.

TEST INFRASTRUCTURE, build container only (needs the reference tree; see oracle/ref_shim.py).  Runs the reference's own
pdf_params, calc_pdf and calc_angles (probability_functions.py:62-96, :8-40, :252-259) and writes numeric arrays only.

Usage:  python scripts/make_prior_golden.py

Maps (in this order): the cnn_response of yud_n120, tiny_n12 and ecd_n300_v8; a map with 7 positive cells; a map with 150
positive cells; the all-zero map (the reference gives NaN weights and density 0 everywhere for it).
Points (the same 300 for every map): 273 seeded uniform points of the square; its corners and edge midpoints at exactly
+-pi/2; ten grid centres, which lie exactly on means; points with |alpha| or |beta| = 3 and 10; one NaN.
Vectors: 60 seeded unit vectors and (0, +-1, 0), (+-1, 0, 0), where calc_angles divides by cos(beta) = 0 or hits the clip.
One mixture that is not pdf_params' (130 components, arbitrary means, some weights 0, negative or NaN) at the first 70
points.
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
REAL = ["yud_n120", "tiny_n12", "ecd_n300_v8"]


def synthetic_map(rng, positive):
    m = np.zeros(400, dtype=np.float32)
    m[rng.choice(400, positive, replace=False)] = rng.uniform(0.01, 1.0, positive).astype(np.float32)
    return m.reshape(20, 20)


def check_cut(m):
    """The 100th and 101st largest values must differ: NumPy's order among equal values belongs to its build.  (Equal
    zeros are no choice at all: whichever of them :87 'removes', the weights are the same.)"""
    v = np.sort(m.ravel())[::-1]
    assert v[99] != v[100] or (v[99] == 0 and v[100] == 0), "the keep-100 cut falls between equal values"


def main():
    warnings.filterwarnings("ignore")
    np.seterr(all="ignore")
    prob = load_reference()["probability_functions"]
    rng = np.random.RandomState(20170327)

    maps = [np.load(os.path.join(GOLDEN, n + ".npz"), allow_pickle=True)["cnn_response"].astype(np.float32) for n in REAL]
    maps += [synthetic_map(rng, 7), synthetic_map(rng, 150), np.zeros((20, 20), dtype=np.float32)]
    for m in maps:
        assert m.shape == (20, 20) and m.dtype == np.float32
        check_cut(m)
    maps = np.stack(maps)

    h = np.pi / 2
    means = prob.pdf_params(maps[0].copy()).means
    pts = np.concatenate([
        rng.uniform(-h, h, (273, 2)),
        [[-h, -h], [-h, h], [h, -h], [h, h]],
        [[-h, 0.0], [h, 0.0], [0.0, -h], [0.0, h]],
        means[rng.choice(400, 10, replace=False)],
        [[3.0, 0.1], [-3.0, 0.1], [0.1, 3.0], [0.1, -3.0], [10.0, 0.1], [-10.0, 0.1], [0.1, 10.0], [0.1, -10.0]],
        [[np.nan, 0.3]],
    ])
    assert pts.shape == (300, 2)

    vecs = rng.standard_normal((60, 3))
    vecs /= np.linalg.norm(vecs, axis=1)[:, None]
    vecs = np.concatenate([vecs, [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]])
    angles = prob.calc_angles(vecs.shape[0], vecs)

    weights, pdf, pdf_vec = [], [], []
    for m in maps:
        before = m.copy()
        par = prob.pdf_params(m)
        assert np.array_equal(m, before) and np.array_equal(par.means, means)
        weights.append(par.weights)
        pdf.append(prob.calc_pdf(par, pts[:, 0], pts[:, 1]))
        pdf_vec.append(prob.calc_pdf(par, angles[:, 0], angles[:, 1]))
    sigma = par.sigma

    arb_means = rng.uniform(-h, h, (130, 2))
    arb_weights = rng.uniform(0.1, 2.0, 130)
    arb_weights[rng.choice(130, 30, replace=False)] = 0.0
    arb_weights[[5, 77]] = -1.0
    arb_weights[[6, 129]] = np.nan
    arb_sigma = 0.2
    arb_pdf = prob.calc_pdf(prob.PDFParams(means=arb_means, weights=arb_weights, sigma=arb_sigma), pts[:70, 0], pts[:70, 1])

    # a directory of its own: the files directly under tests/golden are EM cases to the suite (tests/conftest.py)
    os.makedirs(os.path.join(GOLDEN, "prior"), exist_ok=True)
    out = os.path.join(GOLDEN, "prior", "prior_pdf.npz")
    np.savez_compressed(out, maps=maps, means=means, weights=np.stack(weights), sigma=np.float64(sigma), pts=pts,
                        pdf=np.stack(pdf), vecs=vecs, angles=angles, pdf_vec=np.stack(pdf_vec), arb_means=arb_means,
                        arb_weights=arb_weights, arb_sigma=np.float64(arb_sigma), arb_pdf=arb_pdf)
    w = np.stack(weights)
    print("%s: %d bytes; live components per map %s; NaN densities %d, zero densities %d" % (
        out, os.path.getsize(out), (w > 0).sum(axis=1).tolist(), int(np.isnan(np.stack(pdf)).sum()),
        int((np.stack(pdf) == 0).sum())))


if __name__ == "__main__":
    main()
