"""The split event of the EM: the LDS clustering on the whole workgroup and the E-step + smoother that is left out where a
split event (or the initial compaction) changed nothing.  Both are pure speed choices, so the default is held, bit for
bit, to the forms vpk_em_set_smoother(h, 1) keeps -- the one-wave clustering, every evaluation -- and the clustering to
sklearn as well.

What the whole-EM cases contain, counted with the NumPy oracle (oracle/em_numpy.py: calls of _EM.split that change /
do not change the VP set; whether the compaction behind the initial E-step removes a VP) -- a set without one of the
three classes would hide the branch it is there for:

    16 stored goldens                          4 real splits,  4 no-op splits, initial compaction removes nothing in 2 / 16
    24 scenes of synth.config_scenes(2)        8 real splits, 13 no-op splits, ... in 0 / 24
    scenes 0-2, split_merge_freq 1, 40 it.    10 real splits, 45 no-op splits (scene 1: 10 + 22)
    scenes 0-2, split_merge_freq 3, 40 it.     7 real splits, 11 no-op splits (scene 1:  7 +  4)

The initial compaction removes between 2 and 18 of the 25 initial VPs in every one of the 102 scenes of config 2 (none comes
through with 3 lines each), so extending the scene range does not fill that class: it is the two goldens that start from
given VPs (stress_n300, stress_n1000, init_vp), and stress_n300 is in the time-sliced case below for the same reason.
"""
import warnings

import numpy as np
import pytest

from conftest import golden_cases
from golden_util import em_kwargs, gpu_rasters, load

pytestmark = pytest.mark.gpu

OUTPUTS = ("vp", "sigma", "counts", "counts_weighted", "num_vp", "vp_assoc", "iterations", "status", "flags")
TIE, DISCONNECTED = 1, 2           # include/vpk.h: VPK_EM_FLAG_SPLIT_TIE, VPK_EM_FLAG_SPLIT_DISCONNECTED


# ---- clustering ------------------------------------------------------------------------------------------------------------
def _ldist_of_angles(ang, length=None):
    from oracle import em_numpy as em
    n = ang.shape[0]
    lp = np.stack([np.cos(ang), np.sin(ang), np.zeros(n), np.zeros(n)], 1)
    if length is not None:
        lp = lp * length
    rows = np.repeat(np.arange(n), n).reshape(n, n)
    ld = 1 - em.pair_cosangle(lp, 2, rows, rows.T)
    np.fill_diagonal(ld, 0)
    return ld


def _both_modes(ld):
    """(labels, flags) of the default and of vpk_em_set_smoother(h, 1)"""
    from vanishing_points_2017_amd import kernels
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    new = kernels.cluster2(ld)
    rt.handle.em_set_smoother(1)
    try:
        old = kernels.cluster2(ld)
    finally:
        rt.handle.em_set_smoother(0)
    return new, old


@pytest.fixture(scope="module")
def random_sets():
    """n -> distance matrix, the construction of test_gpu_em.py::test_cluster2_matches_sklearn (one stream of seed 5)"""
    rs = np.random.RandomState(5)
    sets = {}
    for n in (3, 4, 5, 8, 9, 31, 32, 33, 63, 64, 65, 72, 127, 128, 129):
        ang = rs.uniform(0, np.pi, n)
        sets[n] = _ldist_of_angles(ang, rs.uniform(0.1, 1, (n, 1)))
    return sets


# 3: one merge, fewer rows than a trip; 4, 5: the first full trip; 8, 9: the smallest sets a split clusters; 31..33: the cut-over
# from the one-wave to the workgroup body (32), as many rows as eight waves take in one round of trips; 63..65: the second
# block of 64 columns begins; 72: the bench's largest;
# 127, 128: the largest sets the LDS version takes (126 at this panel size, beyond it the global-memory version); 129: beyond
@pytest.mark.parametrize("n", [3, 4, 5, 8, 9, 31, 32, 33, 63, 64, 65, 72, 127, 128, 129])
def test_cluster2_matches_sklearn_and_the_one_wave_form(random_sets, n):
    import sklearn.cluster as cluster
    ld = random_sets[n]
    model = cluster.AgglomerativeClustering(linkage="average", connectivity=ld, n_clusters=2, metric="precomputed")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.fit_predict(ld)
    (labels, flags), (labels1, flags1) = _both_modes(ld.copy())
    assert flags == 0 and flags1 == 0          # random angles: no two candidate merges are exactly tied
    assert np.array_equal(labels, model.labels_)
    assert np.array_equal(labels, labels1)


@pytest.mark.parametrize("reps", [2, 16])      # 8 and 64 lines
def test_cluster2_flags_exact_tie_in_both_forms(reps):
    """four directions over and over (test_gpu_em.py::test_cluster2_flags_exact_tie): the first candidates are exactly tied"""
    ld = _ldist_of_angles(np.tile(np.array([0.0, 0.5, 0.25, 0.75]) * np.pi, reps))
    (labels, flags), (labels1, flags1) = _both_modes(ld)
    assert flags & TIE and flags1 & TIE
    assert flags == flags1
    assert np.array_equal(labels, labels1)


def _three_islands(n):
    """three groups with random distances inside and NO edge between them: n - 3 merges, then the graph is exhausted"""
    rs = np.random.RandomState(n)
    ld = rs.uniform(0.01, 1.0, (n, n))
    ld = np.triu(ld, 1) + np.triu(ld, 1).T
    group = np.arange(n) % 3
    ld[group[:, None] != group[None, :]] = 0.0
    return ld


@pytest.mark.parametrize("case", ["far_apart_9", "far_apart_70", "all_parallel_12", "islands_10", "islands_67", "islands_100"])
def test_cluster2_disconnected_graphs_in_both_forms(case):
    kind, n = case.rsplit("_", 1)
    n = int(n)
    rs = np.random.RandomState(n)
    if kind == "far_apart":        # two groups of directions more than pi / 4 apart: every cross edge is 1 - 6.1e-17
        ang = np.where(np.arange(n) % 2 == 0, rs.uniform(0.0, 0.2, n), rs.uniform(1.4, 1.6, n))
        ld = _ldist_of_angles(ang)
        assert np.all(ld[0::2, 1::2] == 1 - 6.123233995736766e-17)
    elif kind == "all_parallel":   # every distance zero: no edge at all (test_gpu_vp_set.py::test_split_flags_disconnected_and_tie)
        ld = _ldist_of_angles(np.zeros(n))
        assert not ld.any()
    else:
        ld = _three_islands(n)
    (labels, flags), (labels1, flags1) = _both_modes(ld)
    assert flags == flags1
    assert np.array_equal(labels, labels1)
    if kind == "far_apart":        # each group merges within itself (n - 2 merges): the tied cross edges are never the minimum
        assert flags == 0
        assert np.array_equal(labels == labels[0], np.arange(n) % 2 == 0)     # the cut separates the two groups
    else:
        assert flags & DISCONNECTED


# ---- whole EM --------------------------------------------------------------------------------------------------------------
def _host(out):
    return {k: out[k].cpu().numpy() for k in OUTPUTS}


def _run(rt, scenes, mode, **kw):
    from vanishing_points_2017_amd import em as gem
    d = gem.upload_batch(rt, [dict(s, l=s["l"].copy()) for s in scenes])
    rt.handle.em_set_smoother(mode)
    try:
        out = gem.em_batch_device(rt, d["offsets"], d["l"], d["lp"], d["cnn"], d["sphere"], d["init_vp"], gem._params(kw))
        rt.synchronize()
    finally:
        rt.handle.em_set_smoother(0)
    return _host(out)


def _assert_same(got, want):
    for k in OUTPUTS:
        assert np.array_equal(got[k], want[k]), k


@pytest.fixture(scope="module")
def scenes24():
    from vanishing_points_2017_amd import synth
    return gpu_rasters(synth.config_scenes(2, count=24))


@pytest.mark.parametrize("name", golden_cases())
def test_goldens_default_against_every_evaluation(name):
    from vanishing_points_2017_amd.runtime import get_runtime
    g = load(name)
    kw = em_kwargs(g)
    sc = {"l": g["l"], "lp": g["lp"], "cnn_response": g["cnn_response"], "sphere_image": g["sphere_image"],
          "init_vp": kw.pop("init_vp", None)}
    rt = get_runtime(0)
    want = _run(rt, [sc], 1, **kw)
    assert int(want["status"][0]) == int(g["o_status"])
    _assert_same(_run(rt, [sc], 0, **kw), want)


def test_scenes_default_against_every_evaluation(scenes24):
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    want = _run(rt, scenes24, 1)
    assert (want["status"] == 0).all() and want["iterations"].max() > 10      # split events happened
    _assert_same(_run(rt, scenes24, 0), want)


@pytest.mark.parametrize("freq", [1, 3])
def test_a_split_event_every_few_iterations(scenes24, freq):
    """split_merge_freq 1 and 3: the event's two outcomes -- next evaluation left out / kept -- many times per image"""
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    kw = dict(split_merge_freq=freq, num_iter=40)
    want = _run(rt, scenes24[:3], 1, **kw)
    assert (want["status"] == 0).all()
    _assert_same(_run(rt, scenes24[:3], 0, **kw), want)


@pytest.mark.parametrize("freq,slice_ms", [(10, 0.3), (1, 0.15), (3, 0.15), (0, 0.15)])
def test_time_sliced_default_against_uninterrupted_every_evaluation(scenes24, freq, slice_ms):
    """A slice shorter than the set-up, eight launches in flight before the flush: an image is parked at the top of
    iteration 0 (behind the initial evaluation) by its own launch and after every few iterations by the launches that
    follow, so also between a split iteration and the next; a resumed image must evaluate what it finds."""
    from vanishing_points_2017_amd import em as gem
    from vanishing_points_2017_amd.runtime import get_runtime
    if freq == 0:                  # the golden whose initial compaction removes nothing: iteration 0 leaves its evaluation out
        g = load("stress_n300")
        kw = em_kwargs(g)
        scenes = [{"l": g["l"], "lp": g["lp"], "cnn_response": g["cnn_response"], "sphere_image": g["sphere_image"],
                   "init_vp": kw.pop("init_vp")}]
    else:
        scenes = scenes24 if freq == 10 else scenes24[:3]
        kw = {} if freq == 10 else dict(split_merge_freq=freq, num_iter=40)
    want = _run(get_runtime(0), scenes, 1, **kw)
    rt = get_runtime(0, "split_events_slice")
    d = gem.upload_batch(rt, [dict(s, l=s["l"].copy()) for s in scenes])
    rt.handle.em_set_time_slice(slice_ms, int(np.diff(d["offsets"]).max()))
    outs, lines = [], []           # (a launch's lines are normalised in place, by whichever launch starts the image: kept alive)
    try:
        for _ in range(8):
            lines.append(d["l"].clone())
            outs.append(gem.em_batch_device(rt, d["offsets"], lines[-1], d["lp"], d["cnn"], d["sphere"], d["init_vp"],
                                            gem._params(kw)))
        with rt.on_stream():
            rt.handle.em_flush()
        rt.synchronize()
    finally:
        rt.handle.em_set_time_slice(0.0)
    for out in outs:
        _assert_same(_host(out), want)
