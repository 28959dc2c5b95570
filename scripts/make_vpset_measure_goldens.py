"""The REFERENCE's calc_vp_line_counts and merge_vps under "dotprod" and "area" on seeded cases ->
tests/golden/vpset_measures/<measure>_<case>.npz.

TEST INFRASTRUCTURE, build container only (needs the reference tree, scikit-learn, SciPy and joblib; see
oracle/ref_shim.py).  The cases come from tests/vp_set_measure_reference.py (counts_cases, merge_case), which takes the
geometry of tests/vp_set_reference.py and generates only inputs whose every decision has a clear margin in extended
precision; this script asserts it again before it writes.  For a merge it takes the first seeded attempt with clear margins
and the outcome MERGE_OUTCOMES names for the measure, and asserts that the reference's own result has that outcome.
One file per case: the inputs under their own names, the reference's results under ``out_*``, the layout of
tests/golden/vpset.  Arrays only.

  counts  out_counts, out_counts_weighted, out_vp_assoc
  merge   lsim from the reference's calc_lsim (sigma = 1), prior_weights / prior_sigma from its pdf_params;
          out_v (M', 3), out_s, out_kept (the surviving VPs' input indices, read off a second history slice that
          carries them through the reference's np.delete)

Usage:  python scripts/make_vpset_measure_goldens.py
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
import vp_set_reference as R  # noqa: E402
import vp_set_measure_reference as RM  # noqa: E402


def main():
    warnings.filterwarnings("ignore")
    np.seterr(all="ignore")
    mods = load_reference()
    vp, prob = mods["vp_localisation"], mods["probability_functions"]
    os.makedirs(RM.GOLDEN, exist_ok=True)

    for measure in RM.MEASURES:
        for name, c in RM.counts_cases(measure).items():
            assoc = c["vp_assoc"].copy() if "vp_assoc" in c else None
            ref = RM.counts_reference(measure, c["vp"], c["lp"], c["l"], c["s"], c["metric"], c["lweights"], c["thresh"], assoc)
            assert ref[3].clear(), (measure, name)
            cnt, cw, a = vp.calc_vp_line_counts(c["vp"].copy(), c["l"].copy(), c["lp"].copy(), c["s"].copy(), c["metric"].copy(),
                                                c["lweights"].copy(), measure, thresh=float(c["thresh"]), vp_assoc=assoc)
            n = c["lp"].shape[0]
            if n >= RM.INSIDE_FROM_N:
                print("%s %s: the reference counts %d of %d" % (measure, name, int(cnt.sum()), n))
            np.savez_compressed(os.path.join(RM.GOLDEN, "%s_%s.npz" % (measure, name)), out_counts=cnt, out_counts_weighted=cw,
                                out_vp_assoc=np.asarray(a, dtype=np.int64), **c)

        for name in R.MERGE_SPECS:
            want = RM.MERGE_OUTCOMES[measure][name][1:]
            for attempt in range(200):
                c = RM.merge_case(measure, name, attempt)
                cnn = c.pop("cnn")
                par = prob.pdf_params(cnn.copy())
                m = c["v"].shape[0]
                c["lsim"] = vp.calc_lsim(c["lp"].copy(), sigma=1)
                c["prior_weights"] = np.asarray(par.weights, dtype=np.float32)
                c["prior_sigma"] = np.float64(par.sigma)
                ref = RM.merge_reference_of(measure, c)
                if ref["margins"].clear() and R.merge_outcome(ref) == want:
                    break
            else:
                raise AssertionError("no clear %s case for %s" % (measure, name))
            c["attempt"] = np.int64(attempt)
            hist = np.zeros((2, m, 3))
            hist[0] = c["v"]
            hist[1, :, 0] = np.arange(m)
            llen = np.linalg.norm(c["lp"][:, :2] - c["lp"][:, 2:], axis=1)
            res = vp.merge_vps(0, hist, c["s"].copy(), c["l"].copy(), float(c["thresh"]), c["lw"].copy(), c["lsim"].copy(),
                               float(c["wbias"]), par, c["lp"].copy(), llen, measure, max_stdd=float(c["max_stdd"]))
            kept = res["v"][1, :, 0].astype(np.int64)
            assert m - kept.shape[0] == want[0] and np.array_equal(kept, ref["kept"]), (measure, name, kept, ref["kept"])
            if want[1] in ("max_stdd", "none") and not ref["rounds"][-1]["none"]:
                assert (res["s"] != c["s"][kept]).sum() == 1, "a merge given up returns the changed s[k] (:666-668)"
            np.savez_compressed(os.path.join(RM.GOLDEN, "%s_%s.npz" % (measure, name)), out_v=res["v"][0], out_s=res["s"],
                                out_kept=kept, **c)
    print("wrote", len(os.listdir(RM.GOLDEN)), "files to", RM.GOLDEN)


if __name__ == "__main__":
    import joblib
    with joblib.parallel_backend("multiprocessing"):     # the shimmed modules live in memory: forked workers see them
        main()
