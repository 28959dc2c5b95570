"""The REFERENCE's weight_matrix, calc_new_vanishing_point and find_initial_vps on small cases -> tests/golden/emstep/*.npz.

TEST INFRASTRUCTURE, build container only (needs the reference tree; see oracle/ref_shim.py).  Inputs: the first N lines
and M initial VPs of the stored yud_n120 result with its own first-iteration intermediates (i_p_vl0, i_lweight, i_lsim,
i_w0 -- the reference's calc_lsim is not called: its joblib pool cannot pickle the in-memory modules), and the response
maps and sphere images of tests/em_phase_reference.py's init_case.

  weights.npz  per case  <c>_p_vl (M, N), <c>_lweight (N,), <c>_lsim (N, N) and <c>_w_<k> for bias BIASES[k] = 1, 0.001, 0
               N = 1, 2, 3, 12, 65; M = 1, 2, 5
  mstep.npz    per case  <c>_l (N, 3), <c>_w (M, N), <c>_vp (M, 3) and <c>_valid (M,): 0 and a zero row where the
               reference returns None -- an all-zero weight row (:459-460) and an empty one (:456-457, the case n0_m1);
               n1_m1 is one line: LAPACK's reflector
  init.npz     per case  <c>_cnn (20, 20) float32, <c>_sphere (S, S) uint8, <c>_num_max and <c>_v0 (M0, 3): (0, 3) where
               np.vstack raises at :165 (blank: a sphere image with no surviving cell)
Arrays only.

Usage:  python scripts/make_emstep_goldens.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from ref_shim import load_reference  # noqa: E402
import em_phase_reference as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "emstep")
BIASES = (1.0, 0.001, 0.0)
WEIGHT_SHAPES = ((1, 1), (2, 2), (3, 5), (12, 2), (65, 5), (65, 1))
MSTEP_SHAPES = ((1, 1), (2, 2), (3, 1), (12, 3), (65, 5))
INIT_CASES = ((100, 5, "border"), (100, 25, "zero_slice"), (100, 64, "dense"), (100, 25, "blank"), (500, 25, "few"))


def main():
    warnings.filterwarnings("ignore")
    np.seterr(all="ignore")
    vp = load_reference(["coordinate_conversion", "probability_functions", "vp_localisation"])["vp_localisation"]
    y = np.load(os.path.join(ROOT, "tests", "golden", "yud_n120.npz"))
    os.makedirs(GOLDEN, exist_ok=True)

    rec = {}
    for n, m in WEIGHT_SHAPES:
        c = "n%d_m%d" % (n, m)
        p_vl, lw, lsim = y["i_p_vl0"][:m, :n].copy(), y["i_lweight"][:n].copy(), y["i_lsim"][:n, :n].copy()
        rec.update({c + "_p_vl": p_vl, c + "_lweight": lw, c + "_lsim": lsim})
        for k, bias in enumerate(BIASES):
            rec["%s_w_%d" % (c, k)] = vp.weight_matrix(p_vl.copy(), lw.copy(), lsim.copy(), bias=bias)
    np.savez_compressed(os.path.join(GOLDEN, "weights.npz"), **rec)

    rec = {}
    for n, m in MSTEP_SHAPES + ((0, 1),):
        c = "n%d_m%d" % (n, m)
        l, w = y["l_normalised"][:n].copy(), y["i_w0"][:m, :n].copy()
        if (n, m) == (12, 3):
            w[1] = 0.0                                             # np.max(w) == 0 -> None
        out, valid = np.zeros((m, 3)), np.zeros(m, dtype=np.int32)
        for k in range(m):
            v = vp.calc_new_vanishing_point(l.copy(), w[k].copy())
            if v is not None:
                out[k], valid[k] = v, 1
        rec.update({c + "_l": l, c + "_w": w, c + "_vp": out, c + "_valid": valid})
    np.savez_compressed(os.path.join(GOLDEN, "mstep.npz"), **rec)

    rec = {}
    for ssize, num_max, kind in INIT_CASES:
        c = "s%d_%d_%s" % (ssize, num_max, kind)
        cnn, sphere = R.init_case(ssize, num_max, kind)
        try:
            v0 = vp.find_initial_vps(sphere.copy(), cnn.copy(), num_max)
        except ValueError:                                         # np.vstack([]) at :165
            v0 = np.zeros((0, 3))
        rec.update({c + "_cnn": cnn, c + "_sphere": sphere, c + "_num_max": np.int32(num_max), c + "_v0": np.asarray(v0, dtype=np.float64)})
    np.savez_compressed(os.path.join(GOLDEN, "init.npz"), **rec)

    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN))
    assert total < 500000, total
    print("wrote %d files, %d bytes, to %s" % (len(os.listdir(GOLDEN)), total, GOLDEN))


if __name__ == "__main__":
    main()
