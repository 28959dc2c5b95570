"""Run the REFERENCE's own raster + EM + horizon over the KEYWORD surface of expectation_maximisation.

TEST INFRASTRUCTURE, build container only (needs the reference tree; see ref_shim.py).  A sibling of
make_full_goldens.py (whose `instrument` and `save` it uses): that one runs whole configs at the default keywords, this
one runs a few seeded generator scenes under every entry of the keyword table below -- each of the thirteen tunables of
vp_localisation.expectation_maximisation (vp_localisation.py:168-172, mirrored by vpk_em_params) on each side of its
default where both sides mean something, plus combinations -- and writes ONE compact file:

    tests/golden/full_config_keywords.npz      (a "full_c" name: the suite's list of single-run golden cases leaves those out)
        every array of full_c<config>.npz (make_full_goldens.py; one row per (setting, scene) case, no rasters and no
        inputs, only input_sha / raster_sha), with `index` the image index inside `config`, and
        config         BASELINE.json config of the case's scene (seed = 1000 * config + index)
        setting        row of the keyword table the case ran under
        h_status       0 = calc_horizon returned, 1 = it raised on this result (hP1 / hP2 / combo are then zeros / -1)
        setting_names  one label per table row
        kw_names       column names of kw_table: the thirteen keywords, then "init_vp"
        kw_table       [settings, 14] float64, defaults filled in; booleans as 0 / 1; "init_vp" = m > 0 means
                       init_vp = synth.stress_init_vps(seed, m) was supplied
        sig_names / sig_defaults   the reference's keyword names in order and repr() of their defaults, read with
                       inspect.signature from the loaded module ("<required>" for positional arguments)

Only data is written.  Cases run in worker processes (--jobs); each finished case is kept under oracle/_ref/kw_cache/ so
that an interrupted generation resumes (--fresh ignores and overwrites that cache: the check that the committed file
is reproduced).

Usage:  python oracle/make_keyword_goldens.py [--jobs J] [--fresh] [--out PATH]
"""
import inspect
import os
import pickle
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from vanishing_points_2017_amd import synth  # noqa: E402
from vanishing_points_2017_amd.parity import input_sha, raster_sha  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "full_config_keywords.npz")
CACHE = os.path.join(HERE, "_ref", "kw_cache")

KEYWORDS = ("num_iter", "do_merge", "do_split", "do_iterations", "use_weights", "wbias", "num_init_vp", "split_merge_freq",
            "merge_thresh", "outlier_thresh", "final_convergence", "s_thresh", "num_min_lines")

# label, keywords that differ from the defaults ("init_vp": m -> synth.stress_init_vps(seed, m))
SETTINGS = (
    ("no_iterations", dict(do_iterations=False)),
    ("wbias_0.25", dict(wbias=0.25)),
    ("wbias_4", dict(wbias=4.0)),
    ("outlier_1", dict(outlier_thresh=1.0)),
    ("outlier_100", dict(outlier_thresh=100.0)),
    ("min_lines_1", dict(num_min_lines=1)),
    ("min_lines_8", dict(num_min_lines=8)),
    ("init_1", dict(num_init_vp=1)),
    ("init_6", dict(num_init_vp=6)),
    ("init_40", dict(num_init_vp=40)),
    ("init_64", dict(num_init_vp=64)),
    ("freq_1_iter_40", dict(split_merge_freq=1, num_iter=40)),
    ("freq_3", dict(split_merge_freq=3)),
    ("no_split", dict(do_split=False)),
    ("no_merge", dict(do_merge=False)),
    ("converge_5e-2", dict(final_convergence=5e-2)),
    ("forced_12", dict(final_convergence=-1.0, num_iter=12)),
    ("iter_1", dict(num_iter=1)),
    ("iter_7", dict(num_iter=7)),
    ("s_thresh_1e-6", dict(s_thresh=1e-6)),
    ("merge_0.05_freq_4", dict(merge_thresh=0.05, split_merge_freq=4)),
    ("noweights_init_10", dict(use_weights=False, num_init_vp=10)),
    ("initvp_wbias_2_min_5_freq_5", dict(init_vp=8, wbias=2.0, num_min_lines=5, split_merge_freq=5)),
)

# (config, image): three YUD-shape scenes and one ECD-shape scene with N = 662 (> 512 lines: the multi-panel layouts; the
# frequent-split settings take it beyond 32 hypotheses)
SCENES = ((2, 0), (2, 1), (2, 2), (3, 1))
# ... and, for the settings whose keyword changes the outcome on fewer than two of those, scenes on which it does: the
# default run (full_c2.npz) merges on images 39 and 48, splits on 10 and 36, and prunes a VP of fewer than three lines on 4
# and 11 (tests/test_em_keywords.py asserts that every setting's results differ from the default ones on two scenes)
EXTRA_SCENES = {"no_merge": ((2, 39), (2, 48)), "no_split": ((2, 10), (2, 36)), "min_lines_1": ((2, 4), (2, 11))}


def all_cases():
    return [(si, cfg, idx) for si, (name, _) in enumerate(SETTINGS) for cfg, idx in SCENES + EXTRA_SCENES.get(name, ())]


def make_scene(cfg, idx):
    return next(synth.config_scenes(cfg, count=1, start=idx))


def em_kwargs(setting, cfg, idx):
    """Keyword arguments of one table row for one scene, as every implementation takes them."""
    kw = dict(setting)
    m = kw.pop("init_vp", 0)
    if m:
        kw["init_vp"] = synth.stress_init_vps(1000 * cfg + idx, int(m))
    return kw


_STATE = {}


def _worker_setup():
    if _STATE:
        return _STATE
    warnings.filterwarnings("ignore")
    from ref_shim import load_reference
    from make_full_goldens import instrument
    mods = load_reference()
    ev = {"split": 0, "merge": 0, "abort": 0, "final_merge": 0}
    thresh = [1e-3]
    instrument(mods, ev, thresh)            # a list: the wrapper reads the run's merge_thresh at call time
    _STATE.update(mods=mods, ev=ev, thresh=thresh)
    return _STATE


def run_case(args):
    """One (setting, scene) case through the reference: what make_full_goldens.run_config does with a datum."""
    import joblib
    from make_golden import reference_raster
    si, cfg, idx = args
    st = _worker_setup()
    mods, ev = st["mods"], st["ev"]
    vpl, ch = mods["vp_localisation"], mods["calc_horizon"]
    kw = em_kwargs(SETTINGS[si][1], cfg, idx)
    st["thresh"][0] = kw.get("merge_thresh", 1e-3)
    sc = make_scene(cfg, idx)
    sphere = reference_raster(mods["sphere_mapping"], sc["l"])
    for k in ev:
        ev[k] = 0
    n = sc["lp"].shape[0]
    rec = {"index": idx, "config": cfg, "setting": si, "n_lines": n, "input_sha": input_sha(sc),
           "raster_sha": raster_sha(sphere), "raster_sum": int(sphere.sum()), "h_status": 0}
    t0 = time.time()
    status = 0
    with joblib.parallel_backend("multiprocessing"):
        try:
            res = vpl.expectation_maximisation(sc["l"].copy(), sc["lp"].copy(), sc["cnn_response"].copy(),
                                               sphere_image=sphere, **kw)
            if res["vp"] is None:
                status = 1
        except ValueError:
            res, status = None, 2
    rec["ref_seconds"] = time.time() - t0
    rec["status"] = status
    for k in ev:
        rec["ev_" + k] = ev[k]
    rec.update(iterations=0, num_vp=0, assoc=np.full(n, -1, np.int16), hP1=np.zeros(3), hP2=np.zeros(3),
               combo=np.full(3, -1, np.int32))
    if status == 0:
        rec.update(iterations=int(res["iterations"]), num_vp=res["vp"].shape[0], assoc=res["vp_assoc"].astype(np.int16),
                   vp=np.array(res["vp"]), sigma=np.array(res["sigma"]), counts=np.array(res["counts"], dtype=np.float64),
                   counts_w=np.array(res["counts_weighted"], dtype=np.float64))
        try:
            hp1, hp2, _, _, _, combo = ch.calculate_horizon_and_ortho_vp(res, maxbest=20, theta_vmin=np.pi / 10)
            rec.update(hP1=np.asarray(hp1, dtype=np.float64), hP2=np.asarray(hp2, dtype=np.float64),
                       combo=np.asarray(combo, dtype=np.int32))
        except Exception:                   # fewer VPs than the horizon selection can work with
            rec["h_status"] = 1
    print("%-28s c%d #%d N=%d %.1fs status=%d iters=%d M=%d horizon=%d events=%s" % (
        SETTINGS[si][0], cfg, idx, n, rec["ref_seconds"], status, rec["iterations"], rec["num_vp"], rec["h_status"],
        dict(ev)), flush=True)
    return rec


def _cached(case, fresh):
    path = os.path.join(CACHE, "%s_c%d_%d.pkl" % (SETTINGS[case[0]][0], case[1], case[2]))
    if not fresh and os.path.isfile(path):
        with open(path, "rb") as fh:
            return pickle.load(fh)
    rec = run_case(case)
    os.makedirs(CACHE, exist_ok=True)
    with open(path + ".tmp", "wb") as fh:
        pickle.dump(rec, fh)
    os.replace(path + ".tmp", path)
    return rec


def _cached_fresh(case):
    return _cached(case, True)


def _cached_resume(case):
    return _cached(case, False)


def signature(mods):
    names, defaults = [], []
    for name, p in inspect.signature(mods["vp_localisation"].expectation_maximisation).parameters.items():
        names.append(name)
        defaults.append("<required>" if p.default is inspect.Parameter.empty else repr(p.default))
    return np.array(names), np.array(defaults)


def keyword_table(sig_names, sig_defaults):
    import ast
    default = {n: ast.literal_eval(d) for n, d in zip(sig_names, sig_defaults) if n in KEYWORDS}
    names = list(KEYWORDS) + ["init_vp"]
    table = np.zeros((len(SETTINGS), len(names)))
    for r, (_, kw) in enumerate(SETTINGS):
        assert set(kw) <= set(names), kw
        for c, n in enumerate(names):
            table[r, c] = float(kw.get(n, default.get(n, 0)))
    return np.array(names), table


def write(recs, sig, out_path):
    from make_full_goldens import save
    rec = {}
    for r in recs:
        for k, v in r.items():
            rec.setdefault(k, []).append(v)
    for k in ("vp", "sigma", "counts", "counts_w"):
        rec.setdefault(k, [])
    save(rec, out_path)
    out = dict(np.load(out_path, allow_pickle=False))
    for k in ("config", "setting", "h_status"):
        out[k] = np.asarray(rec[k], dtype=np.int32)
    out["setting_names"] = np.array([s[0] for s in SETTINGS])
    out["sig_names"], out["sig_defaults"] = sig
    out["kw_names"], out["kw_table"] = keyword_table(*sig)
    tmp = out_path + ".tmp.npz"
    np.savez_compressed(tmp, **out)
    os.replace(tmp, out_path)


def main(argv):
    from concurrent.futures import ProcessPoolExecutor
    warnings.filterwarnings("ignore")
    jobs, fresh, out_path = 4, False, OUT
    while argv:
        a = argv.pop(0)
        if a == "--jobs":
            jobs = int(argv.pop(0))
        elif a == "--fresh":
            fresh = True
        elif a == "--out":
            out_path = argv.pop(0)
        else:
            raise SystemExit(__doc__)
    cases = all_cases()
    # the large scene's runs first: they are the long ones (the stored order is the table's)
    order = sorted(range(len(cases)), key=lambda k: (cases[k][1] != 3, k))
    t0 = time.time()
    with ProcessPoolExecutor(max_workers=jobs) as pool:
        done = list(pool.map(_cached_fresh if fresh else _cached_resume, [cases[k] for k in order]))
    recs = [None] * len(cases)
    for k, r in zip(order, done):
        recs[k] = r
    from ref_shim import load_reference
    write(recs, signature(load_reference(["coordinate_conversion", "probability_functions", "vp_localisation"])), out_path)
    print("%d cases, %.0f s of reference time, %.0f s wall -> %s (%d bytes)" % (
        len(recs), sum(r["ref_seconds"] for r in recs), time.time() - t0, out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv[1:])
