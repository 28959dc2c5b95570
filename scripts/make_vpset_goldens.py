"""The REFERENCE's calc_vp_line_counts, split_best_vp and merge_vps on seeded cases -> tests/golden/vpset/*.npz.

TEST INFRASTRUCTURE, build container only (needs the reference tree, scikit-learn, SciPy and joblib; see
oracle/ref_shim.py).  The cases come from tests/vp_set_reference.py (counts_cases, split_cases, merge_case), which generates
only inputs whose every decision has a clear margin in extended precision; this script asserts it again before it writes
(for a merge it takes the first seeded attempt with clear margins and the outcome MERGE_SPECS names).
One file per case: the inputs under their own names, the reference's results under ``out_*``.  Arrays only.

  counts  out_counts, out_counts_weighted, out_vp_assoc
  split   out_v (M', 3), out_s, out_split (the VP that was split, or -1), out_labels (N: the labels of scikit-learn's
          clustering for the lines of the worst VP -- captured from the reference's own model object --, -1 elsewhere)
  merge   lsim from the reference's calc_lsim (sigma = 1), prior_weights / prior_sigma from its pdf_params;
          out_v (M', 3), out_s, out_kept (the surviving VPs' input indices, read off a second history slice that
          carries them through the reference's np.delete)

Usage:  python scripts/make_vpset_goldens.py
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from ref_shim import load_reference  # noqa: E402
import vp_set_reference as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "vpset")


def main():
    warnings.filterwarnings("ignore")
    np.seterr(all="ignore")
    mods = load_reference()
    vp, prob = mods["vp_localisation"], mods["probability_functions"]
    os.makedirs(GOLDEN, exist_ok=True)

    for name, c in R.counts_cases().items():
        assoc = c["vp_assoc"].copy() if "vp_assoc" in c else None
        assert R.counts_reference(c["vp"], c["lp"], c["s"], c["metric"], c["lweights"], c["thresh"], assoc)[3].clear(), name
        cnt, cw, a = vp.calc_vp_line_counts(c["vp"].copy(), R._lines_of(c["lp"]), c["lp"].copy(), c["s"].copy(),
                                            c["metric"].copy(), c["lweights"].copy(), "angle", thresh=float(c["thresh"]),
                                            vp_assoc=assoc)
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), out_counts=cnt, out_counts_weighted=cw,
                            out_vp_assoc=np.asarray(a, dtype=np.int64), **c)

    import sklearn.cluster

    class Spy(sklearn.cluster.AgglomerativeClustering):
        seen = None

        def fit_predict(self, X, y=None):
            r = super().fit_predict(X, y)
            Spy.seen = np.array(self.labels_)
            return r

    vp.cluster = types.SimpleNamespace(AgglomerativeClustering=Spy)
    for name, c in R.split_cases().items():
        Spy.seen = None
        m = c["v"].shape[0]
        res = vp.split_best_vp(0, c["v"][None].copy(), c["s"].copy(), c["lp"].copy(), c["l"].copy(), c["w"].copy(),
                               c["lw"].copy(), c["langle"].copy(), min_diff=float(c["min_diff"]))
        v2, s2 = res["v"][0], res["s"]
        split = -1
        if v2.shape[0] > m:
            split = int(np.nonzero((v2[:m] != c["v"]).any(axis=1))[0][0])
        labels = np.full(c["lp"].shape[0], -1, dtype=np.int64)
        if Spy.seen is not None:
            assoc = np.argmax(c["w"], axis=0)
            cand = [k for k in range(m) if (assoc == k).sum() == Spy.seen.shape[0]]
            assert len(cand) == 1, name
            labels[assoc == cand[0]] = Spy.seen
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), out_v=v2, out_s=s2, out_split=np.int64(split),
                            out_labels=labels, **c)

    for name in R.MERGE_SPECS:
        for attempt in range(200):
            c = R.merge_case(name, attempt)
            cnn = c.pop("cnn")
            par = prob.pdf_params(cnn.copy())
            m, n = c["v"].shape[0], c["lp"].shape[0]
            c["lsim"] = vp.calc_lsim(c["lp"].copy(), sigma=1)
            c["prior_weights"] = np.asarray(par.weights, dtype=np.float32)
            c["prior_sigma"] = np.float64(par.sigma)
            ref = R.merge_reference(c["v"], c["s"], c["l"], c["thresh"], c["lw"], c["lsim"], c["wbias"],
                                    (R._grid(), c["prior_weights"], c["prior_sigma"]), c["lp"], float(c["max_stdd"]))
            if ref["margins"].clear() and R.merge_outcome(ref) == R.MERGE_SPECS[name][5:]:
                break
        else:
            raise AssertionError("no clear case for " + name)
        c["attempt"] = np.int64(attempt)
        hist = np.zeros((2, m, 3))
        hist[0] = c["v"]
        hist[1, :, 0] = np.arange(m)
        llen = np.linalg.norm(c["lp"][:, :2] - c["lp"][:, 2:], axis=1)
        res = vp.merge_vps(0, hist, c["s"].copy(), c["l"].copy(), float(c["thresh"]), c["lw"].copy(), c["lsim"].copy(),
                           float(c["wbias"]), par, c["lp"].copy(), llen, "angle", max_stdd=float(c["max_stdd"]))
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), out_v=res["v"][0], out_s=res["s"],
                            out_kept=res["v"][1, :, 0].astype(np.int64), **c)
    print("wrote", len(os.listdir(GOLDEN)), "files to", GOLDEN)


if __name__ == "__main__":
    import joblib
    with joblib.parallel_backend("multiprocessing"):     # the shimmed modules live in memory: forked workers see them
        main()
