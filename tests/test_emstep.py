"""The batched EM update without a GPU: the argument checks of vp_localisation's weight_matrix_batch, mstep_batch,
calc_new_vanishing_point_batch and find_initial_vps_batch (all raised before the runtime is touched), the device code
(csrc/emstep_device.hpp) compiled for the host by tests/hostsim/sim_emstep.cpp and run serially -- one "workgroup" that
takes every image of a ragged batch in turn, in one slot -- against the per-image host build of the single entry points
(tests/hostsim/simlib.py), and the reference's stored results (tests/golden/emstep/) against the extended references.
The kernel itself: tests/test_gpu_emstep.py."""
import ctypes
import os

import numpy as np
import pytest

import em_phase_reference as R
import em_smoother_reference as S
import emstep_cases as C
from hostsim import hostbuild, simlib

HERE = os.path.dirname(os.path.abspath(__file__))

D, L, I = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong), ctypes.c_int
IP, FP, BP = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)

WEIGHT_SHAPES = ((17, 17), (1, 1), (129, 40), (7, 3), (65, 33), (9, 8), (64, 32))
MSTEP_SHAPES = ((15, 5), (1, 1), (65, 33), (2, 4), (64, 64), (3, 32), (129, 4))


@pytest.fixture(scope="module")
def sim():
    lib = hostbuild.load("emstep")
    lib.sim_weight_matrix_batch.argtypes = [I, L, L, D, D, L, D, ctypes.c_double, I, D]
    lib.sim_mstep_batch.argtypes = [I, L, L, D, D, D, D, L, D, ctypes.c_double, ctypes.c_double, D, D, D, IP, IP, D]
    lib.sim_init_vps_batch.argtypes = [I, FP, BP, I, I, D, IP, FP]
    return lib


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def _cat(images, key, dtype=np.float64):
    return np.ascontiguousarray(np.concatenate([np.asarray(im[key], dtype=dtype).ravel() for im in images]))


def _split(buf, lo, vo):
    n, m = np.diff(lo), np.diff(vo)
    at = np.concatenate(([0], np.cumsum(n * m)))
    return [buf[at[b]:at[b + 1]].reshape(m[b], n[b]) for b in range(n.shape[0])]


def sim_weights(sim, images, bias, wt_doubles=0):
    lo, vo = C.offsets(images, "lweight", "p_vl")
    so = np.concatenate(([0], np.cumsum(np.diff(lo) ** 2 + 5))).astype(np.int64)        # (matrices five elements apart)
    lsim = np.full(int(so[-1]), np.nan)
    for b, im in enumerate(images):
        lsim[so[b]:so[b] + im["lsim"].size] = im["lsim"].ravel()
    p_vl, lw = _cat(images, "p_vl"), _cat(images, "lweight")
    w = np.full(p_vl.shape[0], -7.0)
    done = sim.sim_weight_matrix_batch(len(images), _p(lo, L), _p(vo, L), _p(p_vl, D), _p(lw, D), _p(so, L), _p(lsim, D), bias,
                                       wt_doubles, _p(w, D))
    assert done == sum(1 for im in images if im["n"] and im["m"])
    return _split(w, lo, vo)


def sim_mstep(sim, images, mode):
    """mode: 'positions', 'soft' or 'hard'.  Per image (vp, s, err, removed, valid, max_err); outputs pre-filled with -7."""
    lo, vo = C.offsets(images, "l", "cur")
    full = mode != "positions"
    l, w, cur = _cat(images, "l"), _cat(images, "w"), _cat(images, "cur")
    lvsq, p_vl = (_cat(images, "lvsq"), _cat(images, "p_vl")) if full else (None, None)
    assoc = _cat(images, "assoc", np.int64) if mode == "hard" else None
    M, B = int(vo[-1]), len(images)
    vp, s, err = np.full(3 * M, -7.0), np.full(M, -7.0) if full else None, np.full(M, -7.0) if full else None
    removed, valid = np.full(M, -7, np.int32), np.full(M, -7, np.int32)
    mx = np.full(B, -7.0) if full else None
    sim.sim_mstep_batch(B, _p(lo, L), _p(vo, L), _p(l, D), _p(w, D), _p(lvsq, D), _p(p_vl, D), _p(assoc, L), _p(cur, D),
                        R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH, _p(vp, D), _p(s, D), _p(err, D), _p(removed, IP), _p(valid, IP), _p(mx, D))
    out = []
    for b in range(B):
        a, e = int(vo[b]), int(vo[b + 1])
        out.append((vp.reshape(-1, 3)[a:e], None if s is None else s[a:e], None if err is None else err[a:e], removed[a:e],
                    valid[a:e], None if mx is None else mx[b]))
    return out


# ---- argument checks: no GPU, no library ------------------------------------------------------------------------------------
def test_value_errors_need_no_gpu():
    from vanishing_points_2017_amd import vp_localisation as V
    rs = np.random.RandomState(0)
    l, w, lv, p, cur = rs.rand(6, 3), rs.rand(2, 6), rs.rand(6, 2), rs.rand(2, 6), rs.rand(2, 3)
    lw, lsim = rs.rand(6), rs.rand(6, 6)
    with pytest.raises(ValueError, match="describe 2 and 1 images"):
        V.mstep_batch([l, l], [w], [lv], [p], [cur])
    with pytest.raises(ValueError, match="expected"):
        V.mstep_batch([l], [w[:, :5]], [lv], [p], [cur])
    with pytest.raises(ValueError, match="expected"):
        V.mstep_batch([l], [w], [lv.T], [p], [cur])                  # lvsq is (N, M), as PDF.lvsq
    with pytest.raises(ValueError, match="expected"):
        V.mstep_batch([l], [w], [lv], [p], [cur], assocs=[np.zeros(5, np.int64)])
    with pytest.raises(ValueError, match="together"):
        V.mstep_batch([l], [w], [lv], None, [cur])
    with pytest.raises(ValueError, match="together"):
        V.mstep_batch([l], [w], None, [p], [cur])
    with pytest.raises(ValueError, match="at most 64"):
        V.mstep_batch([l], [rs.rand(65, 6)], [rs.rand(6, 65)], [rs.rand(65, 6)], [rs.rand(65, 3)])
    with pytest.raises(ValueError, match="offsets"):
        V.mstep_batch(l, w.ravel(), lv.T.ravel(), p.ravel(), cur)    # concatenated, without offsets
    with pytest.raises(ValueError, match="elements"):
        V.mstep_batch(l, w.ravel()[:-1], lv.T.ravel(), p.ravel(), cur, line_offsets=[0, 6], vp_offsets=[0, 2])
    with pytest.raises(ValueError, match="describe 1 and 2 images"):
        V.calc_new_vanishing_point_batch([l], [w, w])
    with pytest.raises(ValueError, match="expected"):
        V.calc_new_vanishing_point_batch([l[:5]], [w])
    with pytest.raises(ValueError, match="at most 64"):
        V.calc_new_vanishing_point_batch([l], [rs.rand(65, 6)])
    with pytest.raises(ValueError, match="describe 2 and 1 images"):
        V.weight_matrix_batch([p], [lw, lw], [lsim, lsim])
    with pytest.raises(ValueError, match="expected"):
        V.weight_matrix_batch([p[:, :5]], [lw], [lsim])
    with pytest.raises(ValueError, match="one N x N matrix per image"):
        V.weight_matrix_batch([p], [lw], [lsim[:5]])
    with pytest.raises(ValueError, match="one N x N matrix per image"):
        V.weight_matrix_batch([p], [lw], [lsim, lsim])
    with pytest.raises(ValueError, match="at most 64"):
        V.weight_matrix_batch([rs.rand(65, 6)], [lw], [lsim])
    with pytest.raises(ValueError, match="at most 32768"):
        V.calc_new_vanishing_point_batch(np.zeros((32769, 3)), np.zeros(32769), line_offsets=[0, 32769], vp_offsets=[0, 1])
    sph, cnn = np.zeros((2, 40, 40), np.uint8), np.zeros((2, 20, 20), np.float32)
    for num_max in (0, 65):
        with pytest.raises(ValueError, match="1 to 64"):
            V.find_initial_vps_batch(sph, cnn, num_max)
    with pytest.raises(ValueError, match="describe 2 and 1 images"):
        V.find_initial_vps_batch(sph, cnn[:1], 5)
    with pytest.raises(ValueError, match="at least 20"):
        V.find_initial_vps_batch(np.zeros((2, 19, 19), np.uint8), cnn, 5)
    with pytest.raises(ValueError, match="square"):
        V.find_initial_vps_batch([sph[0], np.zeros((41, 41), np.uint8)], cnn, 5)
    with pytest.raises(ValueError, match="20 x 20"):
        V.find_initial_vps_batch(sph, np.zeros((2, 20, 19), np.float32), 5)
    assert V.weight_matrix_batch.__defaults__[0] == 0.001             # the reference's own default (:515)


def test_abi_lists_the_batch_entries():
    from vanishing_points_2017_amd import _lib
    text = open(os.path.join(HERE, "..", "include", "vpk.h")).read()
    for name in ("vpk_weight_matrix_batch", "vpk_mstep_batch", "vpk_init_vps_batch"):
        assert name in _lib.EXPORTS and ("int %s(" % name) in text


# ---- the host build: a ragged batch in one slot == image by image ----------------------------------------------------------
@pytest.mark.parametrize("bias", S.BIASES)
def test_host_weights_batch_equals_singles(sim, bias):
    images = C.weight_images(WEIGHT_SHAPES)
    got = sim_weights(sim, images, bias)
    refs = C.weight_reference(WEIGHT_SHAPES, bias)
    worst = 0.0
    for im, g, ref in zip(images, got, refs):
        if not (im["n"] and im["m"]):
            assert (g == -7.0).all()                                 # nothing of an image without work is written
            continue
        assert np.array_equal(g, simlib.weight_matrix(im["p_vl"], im["lweight"], im["lsim"], bias), equal_nan=True), (im["n"], im["m"])
        worst = max(worst, S.check_smooth(g, ref[0], ref[1], "emstep host batch"))
    print("bias %g: worst error / bar %.3g" % (bias, worst))


def test_host_weights_batch_under_a_small_panel(sim):
    """The LDS budget steers the batch as it steers the single call (vpk_em_set_lds_panel)."""
    images = C.weight_images(WEIGHT_SHAPES)
    for wt in (96, 2048):
        got = sim_weights(sim, images, 1.0, wt)
        for im, g in zip(images, got):
            if im["n"] and im["m"]:
                assert np.array_equal(g, simlib.weight_matrix(im["p_vl"], im["lweight"], im["lsim"], 1.0, lds_doubles=wt), equal_nan=True)


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_host_mstep_batch_equals_singles(sim, mode):
    hard = mode == "hard"
    images = C.mstep_images(MSTEP_SHAPES, hard)
    got = sim_mstep(sim, images, mode)
    worst = 0.0
    for im, (vp, s, err, removed, valid, mx) in zip(images, got):
        if not (im["n"] and im["m"]):
            assert (vp == -7.0).all() and (s == -7.0).all() and (err == -7.0).all() and (removed == -7).all() and (valid == -7).all() and mx == -7.0
            continue
        one = simlib.mstep_full(im["l"], im["w"], im["lvsq"], im["p_vl"], im["cur"], im["assoc32"] if hard else None,
                                R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH)
        for a, b in zip((vp, s, err, removed), one):
            assert np.array_equal(a, b, equal_nan=True), (im["n"], im["m"])
        assert np.array_equal(valid, (s != -1.0).astype(np.int32))
        assert np.array_equal(mx, C.max_err_reference(err), equal_nan=True)
        worst = max(worst, R.check_mstep((vp, s, err, removed), im, im["ref"], im["cur"], hard))
    print("%s: worst error / bar %.3g" % (mode, worst))
    if hard:
        assert any(((im["assoc"] < 0) | (im["assoc"] >= im["m"])).any() for im in images if im["n"] and im["m"])


def test_host_positions_batch_equals_singles(sim):
    images = C.mstep_images(MSTEP_SHAPES, False)
    got = sim_mstep(sim, images, "positions")
    for im, (vp, _, _, removed, valid, _) in zip(images, got):
        if not (im["n"] and im["m"]):
            assert (vp == -7.0).all() and (valid == -7).all()
            continue
        assert np.array_equal(vp, simlib.mstep(im["l"], im["w"]), equal_nan=True)
        none = np.array([rec["kind"] == "none" for rec in im["ref"]])
        assert np.array_equal(valid == 0, none) and (vp[none] == 0).all()


def _sim_init(sim, cases, num_max, weights=True):
    cnn = np.ascontiguousarray(np.stack([c[0] for c in cases]), dtype=np.float32)
    sph = np.ascontiguousarray(np.stack([c[1] for c in cases]), dtype=np.uint8)
    B = len(cases)
    v0, m0 = np.full((B, num_max, 3), -7.0), np.full(B, -7, np.int32)
    wts = np.full((B, 400), -7, np.float32) if weights else None
    sim.sim_init_vps_batch(B, _p(cnn, FP), _p(sph, BP), sph.shape[1], num_max, _p(v0, D), _p(m0, IP), _p(wts, FP))
    return v0, m0, wts


@pytest.mark.parametrize("weights", [True, False], ids=["weights", "no_weights"])
def test_host_init_batch_equals_singles(sim, weights):
    for ssize in (500, 520, 100):
        for num_max in sorted({nm for ss, nm, _ in R.INIT_CASES if ss == ssize}):
            cases = [R.init_case(ss, nm, kind) for ss, nm, kind in R.INIT_CASES if ss == ssize and nm == num_max]
            v0, m0, wts = _sim_init(sim, cases, num_max, weights)
            for b, (cnn, sphere) in enumerate(cases):
                want, w1 = simlib.init_vps(cnn, sphere, num_max)
                assert m0[b] == want.shape[0]
                assert np.array_equal(v0[b, :m0[b]], want) and (v0[b, m0[b]:] == 0).all()
                if weights:
                    assert np.array_equal(wts[b], w1)


# ---- the reference's stored results -------------------------------------------------------------------------------------------
def test_goldens_are_small_and_complete():
    size = sum(os.path.getsize(os.path.join(C.GOLDEN, f)) for f in os.listdir(C.GOLDEN))
    assert sorted(os.listdir(C.GOLDEN)) == ["init.npz", "mstep.npz", "weights.npz"] and size < 500000
    shapes = {C.golden("weights")[c + "_p_vl"].shape for c in C.golden_cases("weights", "_p_vl")}
    assert {n for _, n in shapes} == {1, 2, 3, 12, 65} and {m for m, _ in shapes} == {1, 2, 5}
    g = C.golden("mstep")
    assert list(g["n12_m3_valid"]) == [1, 0, 1] and not g["n12_m3_w"][1].any()      # an all-zero row: None
    assert g["n0_m1_w"].size == 0 and list(g["n0_m1_valid"]) == [0]                  # an empty one: None
    assert g["n1_m1_l"].shape == (1, 3) and g["n1_m1_valid"][0] == 1                 # one line: LAPACK's reflector
    assert C.golden("init")["s100_25_blank_v0"].shape == (0, 3)                      # no surviving cell


def test_weight_goldens_within_the_bound(sim):
    g = C.golden("weights")
    cases = C.golden_cases("weights", "_p_vl")
    images = [{"p_vl": g[c + "_p_vl"], "lweight": g[c + "_lweight"], "lsim": g[c + "_lsim"], "n": g[c + "_lweight"].shape[0],
               "m": g[c + "_p_vl"].shape[0]} for c in cases]
    for k, bias in enumerate(S.BIASES):
        got = sim_weights(sim, images, bias)
        for c, im, w_sim in zip(cases, images, got):
            w, bar = S.smooth_reference(im["p_vl"] * im["lweight"][None, :], 0 * im["p_vl"], im["lweight"], im["lsim"], bias)
            r0 = S.check_smooth(g["%s_w_%d" % (c, k)], w, bar, "emstep golden")
            r1 = S.check_smooth(w_sim, w, bar, "emstep host on golden")
            print("%s bias %g: reference / host build error over bar %.3g / %.3g" % (c, bias, r0, r1))


def test_mstep_goldens_against_the_extended_reference(sim):
    g = C.golden("mstep")
    cases = [c for c in C.golden_cases("mstep", "_vp")]
    images = []
    for c in cases:
        l, w = g[c + "_l"], g[c + "_w"]
        m, n = w.shape
        images.append({"l": l, "w": w, "cur": np.zeros((m, 3)), "n": n, "m": m})
    got = sim_mstep(sim, images, "positions")
    for c, im, (vp, _, _, _, valid, _) in zip(cases, images, got):
        want, ok = g[c + "_vp"], g[c + "_valid"]
        if im["n"] == 0:
            assert (valid == -7).all() and not ok.any()            # the empty row: None there, no work here
            continue
        assert np.array_equal(valid, ok)
        ones = np.ones_like(im["w"])
        ref = R.mstep_reference(im["l"], im["w"], ones, ones, None)
        for k, rec in enumerate(ref):
            if rec["kind"] == "none":
                assert ok[k] == 0 and (vp[k] == 0).all()
                continue
            for name, x in (("reference", want[k]), ("host build", vp[k])):
                if rec["kind"] == "one":
                    assert np.abs(x - R.lapack_one_row(im["l"][0])).max() <= 1e-14, (c, k, name)
                else:
                    s1, s2, s3 = rec["sv"]
                    assert float(R.residual(im["l"], rec["r"], x)) <= float(rec["res_bound"]), (c, k, name)
                    if s2 > R.c_of_n(im["n"]) * R.U * s1 * 4:
                        e = np.sqrt(((R.ld(x) - rec["vp"]) ** 2).sum())
                        assert e <= rec["vec_bound"], (c, k, name, float(e), float(rec["vec_bound"]))


def test_init_goldens(sim):
    from oracle import em_numpy as em
    g = C.golden("init")
    for c in C.golden_cases("init", "_v0"):
        cnn, sphere, num_max, want = g[c + "_cnn"], g[c + "_sphere"], int(g[c + "_num_max"]), g[c + "_v0"]
        v0, m0, wts = _sim_init(sim, [(cnn, sphere), (cnn, sphere)], num_max)
        for b in (0, 1):                                             # (the same image twice: the second in a used workgroup)
            assert m0[b] == want.shape[0] and (v0[b, m0[b]:] == 0).all()
            if want.size:
                assert np.abs(v0[b, :m0[b]] - want).max() <= 1e-13
            assert np.array_equal(wts[b], em.pdf_params(cnn.copy()).weights)
