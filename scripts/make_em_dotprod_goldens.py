"""The REFERENCE's expectation_maximisation under distance_measure="dotprod" -> tests/golden/em_dotprod/*.npz.

TEST INFRASTRUCTURE, build container only (needs the reference tree; see oracle/ref_shim.py).  Inputs are the stored
tests/golden/<case>.npz (lines, response, raster, keywords, init_vp); nothing of them is stored again.  A file named
``<case>__<variant>.npz`` runs <case> with the keywords it carries itself (``kw_*`` / ``init_vp``, or ``drop_init_vp``: without
the stored init_vp) laid over the stored ones.
Per file, arrays only: the ``o_*`` fields tests/golden_util.check_em_result reads, and ``d_lvsq`` (N, M) / ``d_p_vl`` (M, N),
the last E-step's lvsq and p_vl from EM_result['distribution'].

Stability gate: every case runs three times -- as stored, and with one coordinate of ``lp`` moved by one ulp at two
different places -- and is REFUSED (nothing written) when the runs differ in iterations, VP count or any assignment.

Outlier margin: the HIP path tests sqrt(lvsq) where calc_vp_line_counts (:496) tests |vp . l|, equal to within an ulp;
every outlier test of every recorded run must therefore stay clear of its threshold by 1e-9 relative, which is asserted.

Usage:  python scripts/make_em_dotprod_goldens.py [file stem ...]
"""
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

from ref_shim import load_reference  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "em_dotprod")
OUTLIER_MARGIN = 1e-9

# file stem -> keywords laid over the stored case's (the part of the stem before "__")
CASES = {
    "tiny_n12": {}, "clean3_n60": {}, "noweights_n100": {}, "yud_n120": {}, "nosplit_n150": {}, "yud_n200": {},
    "mergeabort_n200": {}, "periodicmerge_n220": {}, "yud_n250": {}, "ecd_n300_v8": {}, "stress_n300": {}, "stress_n1000": {},
    # merge and split run under the measure every third iteration
    "yud_n200__freq3": {"split_merge_freq": 3},
    # init_vp given (:212-215): the scene's true VPs and two directions no line supports, none of them normalised
    "yud_n120__initvp": {"init_vp": "true_vps"},
    # the stress scenes from find_initial_vps' 25 candidates instead of their stored init_vp (the file carries drop_init_vp):
    # 18 and 24 final VPs where the stored eight initial VPs leave 7 and 8
    "stress_n300__noinit": {"init_vp": None},
    "stress_n1000__noinit": {"init_vp": None},
}


def stored_inputs(stem, extra):
    base = stem.split("__")[0]
    g = dict(np.load(os.path.join(GOLDEN, base + ".npz"), allow_pickle=False))
    kw = {k[3:]: (g[k].item() if g[k].ndim == 0 else g[k]) for k in g if k.startswith("kw_")}
    if "init_vp" in g:
        kw["init_vp"] = g["init_vp"]
    carried = {}
    for k, v in extra.items():
        if k == "init_vp" and v is None:
            carried["drop_init_vp"] = np.array(1)
            kw.pop("init_vp", None)
            continue
        if k == "init_vp":
            v = np.vstack([2.0 * g["true_vps"], [[0.3, -0.2, 0.9], [-0.7, 0.1, 0.4]]])
            carried["init_vp"] = v
        else:
            carried["kw_" + k] = np.array(v)
        kw[k] = v
    return g, kw, carried


def nudged(lp, which):
    lp = lp.copy()
    if which == 1:
        lp[0, 0] = np.nextafter(lp[0, 0], np.inf)
    elif which == 2:
        lp[lp.shape[0] // 2, 3] = np.nextafter(lp[lp.shape[0] // 2, 3], -np.inf)
    return lp


def watched(inner, worst):
    """The reference's calc_vp_line_counts, noting in worst[0] the smallest relative distance of a tested line to its threshold."""

    def wrapped(vp, l, lp, s, decision_metric, lweights, distance_measure, thresh=2.57, vp_assoc=None):
        assoc = np.argmax(decision_metric, axis=0) if vp_assoc is None else vp_assoc
        for n in range(l.shape[0]):
            m = assoc[n]
            if m > -1 and distance_measure == "dotprod":
                dist = np.abs(np.dot(vp[m], l[n, :]))
                t = thresh * np.sqrt(s[m])
                worst[0] = min(worst[0], abs(dist - t) / t)
        return inner(vp, l, lp, s, decision_metric, lweights, distance_measure, thresh=thresh, vp_assoc=vp_assoc)

    return wrapped


def run_case(stem, extra, vpl, counts_fn):
    import joblib
    g, kw, carried = stored_inputs(stem, extra)
    runs = []
    worst = [np.inf]
    vpl.calc_vp_line_counts = watched(counts_fn, worst)
    t0 = time.time()
    for which in range(3):
        l = g["l"].copy()
        k = {a: (b.copy() if isinstance(b, np.ndarray) else b) for a, b in kw.items()}
        with joblib.parallel_backend("multiprocessing"):
            res = vpl.expectation_maximisation(l, nudged(g["lp"], which), g["cnn_response"].copy(),
                                               sphere_image=g["sphere_image"], distance_measure="dotprod", **k)
        runs.append(res)
    dt = (time.time() - t0) / 3
    r0 = runs[0]
    for r in runs[1:]:
        same = (r["vp"] is None) == (r0["vp"] is None)
        if same and r0["vp"] is not None:
            same = (r["iterations"] == r0["iterations"] and r["vp"].shape == r0["vp"].shape and
                    np.array_equal(r["vp_assoc"], r0["vp_assoc"]))
        if not same:
            print("%-24s REFUSED: the reference's own runs differ under a one-ulp nudge" % stem)
            return 0
    assert worst[0] > OUTLIER_MARGIN, (stem, worst[0])
    out = dict(carried)
    if r0["vp"] is None:
        out["o_status"] = np.array(1)
    else:
        d = r0["distribution"]
        out.update(o_status=np.array(0), o_vp=r0["vp"], o_vp_assoc=r0["vp_assoc"], o_counts=r0["counts"],
                   o_counts_weighted=r0["counts_weighted"], o_sigma=r0["sigma"], o_iterations=np.array(r0["iterations"]),
                   d_lvsq=np.asarray(d.lvsq, dtype=np.float64), d_p_vl=np.asarray(d.vl, dtype=np.float64),
                   vp_spread=np.array(max(np.abs(r["vp"] - r0["vp"]).max() for r in runs[1:])),
                   outlier_margin=np.array(worst[0]))
    path = os.path.join(OUT, stem + ".npz")
    np.savez_compressed(path, **out)
    print("%-24s N=%4d  %.1fs/run  iters=%s  M=%s  vp spread %.1e  outlier margin %.1e  %d bytes" % (
        stem, g["lp"].shape[0], dt, r0["iterations"], None if r0["vp"] is None else r0["vp"].shape[0],
        float(out.get("vp_spread", 0)), worst[0], os.path.getsize(path)))
    return os.path.getsize(path)


def main(argv):
    warnings.filterwarnings("ignore")
    np.seterr(all="ignore")
    vpl = load_reference()["vp_localisation"]
    os.makedirs(OUT, exist_ok=True)
    counts_fn = vpl.calc_vp_line_counts
    for stem in (argv or list(CASES)):
        run_case(stem, CASES[stem], vpl, counts_fn)
    size = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print("%d files, %d bytes, in %s" % (len(os.listdir(OUT)), size, OUT))


if __name__ == "__main__":
    main(sys.argv[1:])
