"""Every keyword of expectation_maximisation against the REFERENCE's own results, without a GPU.

tests/golden/full_config_keywords.npz holds what the reference made of a few generator scenes under every row of a
keyword table (oracle/make_keyword_goldens.py: each of the thirteen tunables of vp_localisation.py:168-172 away from its
default, on both sides where both mean something, plus combinations; three YUD-shape scenes and one ECD-shape scene of
662 lines, which the frequent-split rows take beyond 32 hypotheses).  Held to it here, at the bar of every other parity
test (parity.compare_one / parity.passes: status, iteration count, VP count, assignments bit-exact, per-VP counts, VP
directions within parity.VP_TOL):

* the CPU oracle (oracle/em_numpy.py), which the "fresh scenes" GPU tests trust, and
* the EM device source compiled for the host (tests/hostsim): a device-code bug under a keyword shows here.

A case may miss the bar only with a certificate (tests/golden/instability_keywords.npz: one-ulp reruns of the reference
itself under that row's keywords, oracle/make_instability_certificates.py --keywords), handled as
test_gpu_full_configs handles certified images (golden_util.check_parity); certificates may cover at most one case in
ten, and every row needs two cases that meet the bar outright.  The -m gpu counterpart is test_gpu_em_keywords.py.
"""
import ast
import inspect

import numpy as np
import pytest

from golden_util import check_parity, cpu_rasters
from vanishing_points_2017_amd import parity

REF = parity.KeywordResults()
SETTINGS = REF.setting_names
CERT = parity.keyword_instability_certificates()
KEYWORDS = tuple(str(n) for n in REF.g["kw_names"][:-1])     # the table's columns (test_c_abi_defaults: vpk_em_params' fields)
_SCENES = {}


def scene_of(row):
    """The row's generator scene with the raster the oracle's Agg restatement makes of its lines, checked against the hashes
    of what the reference saw."""
    key = (int(REF.config[row]), int(REF.index[row]))
    if key not in _SCENES:
        sc = cpu_rasters([REF.scene(row)])[0]
        g = REF.get(row)
        assert parity.input_sha(sc) == g["input_sha"], "the generator produced other inputs than the reference saw"
        assert parity.raster_sha(sc["sphere_image"]) == g["raster_sha"]
        _SCENES[key] = sc
    return _SCENES[key]


def label(setting, row):
    return (setting, int(REF.config[row]), int(REF.index[row]))


def hold_to_the_bar(setting, run):
    """run(scene, **kw) -> result dict with 'status'.  The caps that keep a certificate from carrying a setting."""
    items = []
    for row in REF.rows(setting):
        sc = scene_of(row)
        items.append((label(setting, row), run(sc, **REF.kwargs(setting, row)), REF.get(row), CERT.get(label(setting, row))))
    outright, excused, bad = check_parity(items)
    assert not bad, "%s: misses the parity bar without an instability certificate: %s" % (setting, bad)
    assert len(outright) >= 2, (setting, outright, excused)


def test_the_table_covers_every_keyword_and_the_large_regimes():
    names = [str(n) for n in REF.g["kw_names"]]
    assert tuple(names[:-1]) == KEYWORDS and names[-1] == "init_vp"
    table = REF.g["kw_table"]
    default = {str(n): ast.literal_eval(str(d)) for n, d in zip(REF.g["sig_names"], REF.g["sig_defaults"]) if str(d) != "<required>"}
    for c, n in enumerate(KEYWORDS):                                       # every tunable leaves its default somewhere
        assert (table[:, c] != float(default[n])).any(), n
    for n in ("wbias", "outlier_thresh", "num_min_lines", "num_init_vp", "split_merge_freq", "final_convergence", "s_thresh",
              "merge_thresh", "num_iter"):
        c = KEYWORDS.index(n)                                              # ... on both sides where both mean something
        assert (table[:, c] < float(default[n])).any() or n in ("s_thresh", "merge_thresh"), n
        assert (table[:, c] > float(default[n])).any() or n in ("split_merge_freq", "num_iter"), n
    assert (table[:, -1] > 0).any()                                        # a supplied init_vp
    single = [KEYWORDS.index("do_split"), KEYWORDS.index("do_merge")]
    assert any(r[single[0]] == 0 and r[single[1]] == 1 for r in table) and any(r[single[0]] == 1 and r[single[1]] == 0 for r in table)
    per_setting = np.bincount(REF.setting, minlength=len(SETTINGS))
    assert per_setting.min() >= 3 and len(REF) == per_setting.sum()
    big = REF.g["n_lines"] > 512
    assert big.sum() >= 2 and REF.g["num_vp"][big].max() > 32              # the regime beyond the 32 accumulators
    freq = table[REF.setting, KEYWORDS.index("split_merge_freq")]
    assert (big & (freq < 10) & (REF.g["num_vp"] > 32)).sum() >= 2


def test_every_setting_changes_the_outcome_on_two_scenes():
    """A keyword that changes nothing on the chosen scenes is not tested by them: under every setting the reference's stored
    result must miss the parity bar against the reference's DEFAULT-keyword result of the same scene (full_c2 / full_c3) on at
    least two scenes -- do_merge=False needs scenes whose default run merges, do_split=False ones whose default run splits."""
    default = {cfg: parity.ReferenceResults(cfg) for cfg in sorted(set(int(c) for c in REF.config))}
    for setting in SETTINGS:
        differs = [row for row in REF.rows(setting) if not parity.passes(parity.compare_one(
            REF.get(row), default[int(REF.config[row])].get(int(REF.index[row]))))]
        assert len(differs) >= 2, (setting, [label(setting, row) for row in differs])


def test_certificates_cover_at_most_one_case_in_ten():
    rows = {label(SETTINGS[int(REF.setting[k])], k) for k in range(len(REF))}
    unstable = [k for k, c in CERT.items() if c["unstable"]]
    assert set(unstable) <= rows
    assert len(unstable) * 10 <= len(rows), (len(unstable), len(rows))


@pytest.mark.parametrize("setting", SETTINGS)
def test_oracle_meets_the_bar_under_every_keyword_setting(setting):
    from oracle import em_numpy

    def run(sc, **kw):
        try:
            res = em_numpy.expectation_maximisation(sc["l"].copy(), sc["lp"].copy(), sc["cnn_response"].copy(),
                                                    sphere_image=sc["sphere_image"], **kw)
        except ValueError:
            return {"status": 2, "flags": 0}
        return dict(res, status=0 if res["vp"] is not None else 1, flags=0)      # (no capacity limits in the oracle: no flags)
    hold_to_the_bar(setting, run)


@pytest.mark.parametrize("setting", SETTINGS)
def test_host_build_of_the_device_code_meets_the_bar_under_every_keyword_setting(setting):
    from hostsim import simlib

    def run(sc, **kw):
        return simlib.em_single(sc["l"].copy(), sc["lp"], sc["cnn_response"], sc["sphere_image"], **kw)
    hold_to_the_bar(setting, run)


def _reference_signature():
    return [(str(n), str(d)) for n, d in zip(REF.g["sig_names"], REF.g["sig_defaults"])]


@pytest.mark.parametrize("which", ["product", "oracle"])
def test_python_signatures_mirror_the_reference(which):
    """Names, order and defaults of the reference's expectation_maximisation, as read from it when the golden was made.  The
    product and the oracle may only append arguments of their own behind them."""
    if which == "product":
        from vanishing_points_2017_amd import vp_localisation as mod
    else:
        from oracle import em_numpy as mod
    ours = list(inspect.signature(mod.expectation_maximisation).parameters.items())
    want = _reference_signature()
    assert len(want) == 19 and len(ours) >= len(want)
    for (name, p), (rname, rdefault) in zip(ours, want):
        assert name == rname
        if rdefault == "<required>":
            assert p.default is inspect.Parameter.empty, name
        else:
            d = ast.literal_eval(rdefault)
            assert p.default == d and isinstance(p.default, bool) == isinstance(d, bool), (name, p.default, d)


def test_c_abi_defaults_mirror_the_reference():
    """vpk_em_default_params (include/vpk.h: vpk_em_params) and the host build's copy carry the reference's defaults for
    every tunable; the struct has no field the reference does not have."""
    import os
    from hostsim import simlib
    from vanishing_points_2017_amd import _lib
    want = {n: ast.literal_eval(d) for n, d in _reference_signature() if n in KEYWORDS}
    assert set(want) == set(KEYWORDS)
    assert os.path.exists(_lib.SO_PATH), "libvpk.so is not built: vpk_em_default_params cannot be compared"
    for p in (simlib.default_params(), _lib.default_em_params()):
        assert {f for f, _ in p._fields_} == set(KEYWORDS)
        for n in KEYWORDS:
            assert getattr(p, n) == want[n], (n, getattr(p, n), want[n])
