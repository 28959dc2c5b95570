"""The REFERENCE's calc_probabilities with its three distance measures on seeded cases -> tests/golden/estep/*.npz.

TEST INFRASTRUCTURE, build container only (needs the reference tree; see oracle/ref_shim.py).  Inputs: the lines, final
VPs and variances of the stored yud_n120, clean3_n60 and tiny_n12 results (at most 65 lines and 5 VPs of each), a VP at
infinity (v[2] = 0: a NaN column for "angle" and "area", finite for "dotprod"), a variance of 0 (the 1e-200 floor), one
line against one VP, and the arbitrary 130-component mixture of tests/golden/prior/prior_pdf.npz as one case's prior.
Each case runs with two variance vectors per measure: ``s_<measure>_0`` the EM's own -- with which nearly every line of
"dotprod" and "area" sits on the 1e-12 floor of p_l -- and ``s_<measure>_1`` = median_n(lvsq[n, m]) / 2.
One file per case: the inputs under their own names (lp, l, v, means, weights, sigma, s_*), the reference's results under
``out_<measure>_<k>_<field>`` with field one of p_v, angles, lvsq, p_lv, p_l, p_vl, s (the floored variances :139).  Arrays only.

Usage:  python scripts/make_estep_goldens.py
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "estep")
MEASURES = ("angle", "dotprod", "area")


def stored(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return {k: z[k] for k in ("l_normalised", "lp", "o_vp", "o_sigma", "cnn_response")}


def cases(prob):
    arb = np.load(os.path.join(ROOT, "tests", "golden", "prior", "prior_pdf.npz"))
    out = {}
    y = stored("yud_n120")
    par = prob.pdf_params(y["cnn_response"].copy())
    out["yud_n65_m5"] = dict(lp=y["lp"][:65], l=y["l_normalised"][:65], v=y["o_vp"][:5], s=y["o_sigma"][:5], par=par)
    c = stored("clean3_n60")
    par = prob.pdf_params(c["cnn_response"].copy())
    out["clean3_n60_m4_infinite_vp"] = dict(lp=c["lp"], l=c["l_normalised"], v=np.vstack([c["o_vp"], [0.6, 0.8, 0.0]]),
                                            s=np.append(c["o_sigma"], 1e-4), par=par)
    t = stored("tiny_n12")
    par = prob.PDFParams(means=arb["arb_means"], weights=arb["arb_weights"], sigma=float(arb["arb_sigma"]))
    out["tiny_n12_m2_zero_s_mixture130"] = dict(lp=t["lp"], l=t["l_normalised"], v=t["o_vp"], s=np.array([0.0, t["o_sigma"][1]]),
                                               par=par)
    par = prob.pdf_params(t["cnn_response"].copy())
    out["tiny_n1_m1"] = dict(lp=t["lp"][:1], l=t["l_normalised"][:1], v=t["o_vp"][:1], s=t["o_sigma"][:1], par=par)
    return out


def main():
    warnings.filterwarnings("ignore")
    np.seterr(all="ignore")
    prob = load_reference(["probability_functions"])["probability_functions"]
    os.makedirs(GOLDEN, exist_ok=True)
    total = 0
    for name, c in cases(prob).items():
        lp, l, v = (np.ascontiguousarray(c[k], dtype=np.float64) for k in ("lp", "l", "v"))
        par = c["par"]
        rec = {"lp": lp, "l": l, "v": v, "means": np.asarray(par.means, dtype=np.float64), "weights": np.asarray(par.weights),
               "sigma": np.float64(par.sigma)}
        llen = np.linalg.norm(lp[:, :2] - lp[:, 2:], axis=1)
        for meas in MEASURES:
            fn = {"angle": prob.calc_lvsq_angle, "dotprod": prob.calc_lvsq_dotprod, "area": prob.calc_lvsq_area}[meas]
            lvsq = fn(v.T.copy(), l.copy(), lp.copy(), llen)
            med = np.median(lvsq, axis=0) / 2
            s1 = np.where(np.isfinite(med) & (med > 0), med, 1e-4)
            for k, s in enumerate((np.asarray(c["s"], dtype=np.float64), s1)):
                rec["s_%s_%d" % (meas, k)] = s.copy()
                sw = s.copy()
                pdf = prob.calc_probabilities(0, par, v[None].copy(), l.copy(), lp.copy(), sw, llen, distance_measure=meas)
                for field, val in (("p_v", pdf.v), ("angles", pdf.angles), ("lvsq", pdf.lvsq), ("p_lv", pdf.lv), ("p_l", pdf.l),
                                   ("p_vl", pdf.vl), ("s", sw)):
                    rec["out_%s_%d_%s" % (meas, k, field)] = np.asarray(val, dtype=np.float64)
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, **rec)
        total += os.path.getsize(path)
    assert total < 500000, total
    print("wrote %d files, %d bytes, to %s" % (len(os.listdir(GOLDEN)), total, GOLDEN))


if __name__ == "__main__":
    main()
