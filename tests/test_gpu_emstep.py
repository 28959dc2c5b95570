"""The batched EM update on the GPU (csrc/vpk_emstep.hip): vpk_weight_matrix_batch, vpk_mstep_batch, vpk_init_vps_batch and
their vp_localisation wrappers.  Every family runs as ONE ragged launch, out of size order and interleaved with images that
have no lines or no VPs, and is held

  1. bit for bit to the single-image entry points (kernels.weight_matrix / mstep_full / mstep / init_vps), also with the
     grid capped at two workgroups (vpk_em_set_workgroups(2)): every workgroup then takes several images, one after the
     other, in one slot -- the path a single-image call never reaches;
  2. to the extended-precision references of tests/em_smoother_reference.py and tests/em_phase_reference.py;
  3. to the reference's own stored intermediates;
  4. in composition: a whole iteration from device-resident calls equals the same calls fed host copies;
  5. to the EM's own decision metric;
  6. at the C-ABI: every error case returns its status and leaves the outputs alone.
The inputs are those of tests/test_emstep.py (tests/emstep_cases.py), which runs the host build of the same device code."""
import ctypes
import functools

import numpy as np
import pytest

import em_phase_reference as R
import em_smoother_reference as S
import emstep_cases as C
from golden_util import abserr, em_kwargs, load, relerr
from oracle import em_numpy as em

pytestmark = pytest.mark.gpu

# the shapes of CPU_SHAPES up to (257, 64) -- the 8-slice range --, (449, 20) sparse-eligible, (897, 8) single-chain; mixed in size
_W = [s for s in S.CPU_SHAPES if s[0] <= 257] + [(449, 20), (897, 8)]
WEIGHT_SHAPES = tuple(_W[i] for i in (3, 9, 0, 6, 10, 1, 8, 4, 2, 7, 5))
MSTEP_SHAPES = tuple(R.mstep_shapes()[i] for i in np.random.RandomState(3).permutation(len(R.mstep_shapes())))
INTERMEDIATES = ("clean3_n60", "mergeabort_n200", "nosplit_n150", "periodicmerge_n220", "tiny_n12", "yud_n120", "yud_n200", "yud_n250")


def _handle():
    from vanishing_points_2017_amd.runtime import get_runtime
    return get_runtime(0).handle


def _with(workgroups, smoother, fn):
    h = _handle()
    h.em_set_workgroups(workgroups)
    h.em_set_smoother(smoother)
    try:
        return fn()
    finally:
        h.em_set_workgroups(0)
        h.em_set_smoother(0)


def _np(x):
    return x.cpu().numpy()


def _work(im):
    return im["n"] > 0 and im["m"] > 0


# ---- 1 + 2: weights -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single_weights(bias, smoother):
    from vanishing_points_2017_amd import kernels
    return _with(0, smoother, lambda: [kernels.weight_matrix(im["p_vl"], im["lweight"], im["lsim"], bias) if _work(im) else None
                                       for im in C.weight_images(WEIGHT_SHAPES)])


@pytest.mark.parametrize("workgroups", [0, 2], ids=["grid", "two_workgroups"])
@pytest.mark.parametrize("bias", S.BIASES)
def test_weights_batch(bias, workgroups):
    from vanishing_points_2017_amd import vp_localisation as V
    images = C.weight_images(WEIGHT_SHAPES)
    assert sum(_work(im) for im in images) >= 7 and sum(not _work(im) for im in images) >= 3
    refs = C.weight_reference(WEIGHT_SHAPES, bias)
    for smoother in (0, 1):
        got = _with(workgroups, smoother, lambda: V.weight_matrix_batch([im["p_vl"] for im in images], [im["lweight"] for im in images],
                                                                        [im["lsim"] for im in images], bias=bias))
        worst = 0.0
        for im, g, one, ref in zip(images, got, single_weights(bias, smoother), refs):
            assert tuple(g.shape) == (im["m"], im["n"])
            if not _work(im):
                continue
            assert np.array_equal(_np(g), one, equal_nan=True), "N=%d M=%d smoother %d: other bits than vpk_weight_matrix" % (im["n"], im["m"], smoother)
            worst = max(worst, S.check_smooth(_np(g), ref[0], ref[1], "emstep batch"))
        print("weights bias %g workgroups %d smoother %d: worst error / bar %.3g" % (bias, workgroups, smoother, worst))


# ---- 1 + 2: M-step ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single_mstep(hard):
    from vanishing_points_2017_amd import kernels
    return [kernels.mstep_full(im["l"], im["w"], im["lvsq"], im["p_vl"], im["cur"], im["assoc32"] if hard else None,
                               R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH) if _work(im) else None for im in C.mstep_images(MSTEP_SHAPES, hard)]


@pytest.mark.parametrize("workgroups", [0, 2], ids=["grid", "two_workgroups"])
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
def test_mstep_batch(hard, workgroups):
    from vanishing_points_2017_amd import vp_localisation as V
    images = C.mstep_images(MSTEP_SHAPES, hard)
    assert sum(_work(im) for im in images) >= 7 and sum(not _work(im) for im in images) >= 3
    r = _with(workgroups, 0, lambda: V.mstep_batch([im["l"] for im in images], [im["w"] for im in images], [im["lvsq"].T for im in images],
                                                   [im["p_vl"] for im in images], [im["cur"] for im in images],
                                                   [im["assoc"] for im in images] if hard else None, R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH))
    v, s, err, removed, valid, mx = (_np(r[k]) for k in ('v', 's', 'err', 'removed', 'valid', 'max_err'))
    vo = r['vp_offsets']
    worst = 0.0
    for b, (im, one) in enumerate(zip(images, single_mstep(hard))):
        a, e = int(vo[b]), int(vo[b + 1])
        if not _work(im):
            assert (v[a:e] == 0).all() and (s[a:e] == -1).all() and (err[a:e] == -1).all() and not removed[a:e].any() and mx[b] == 0
            continue
        out = (v[a:e], s[a:e], err[a:e], removed[a:e])
        for x, y, name in zip(out, one, ("vp", "s", "err", "removed")):
            assert np.array_equal(x, y, equal_nan=True), "N=%d M=%d: %s has other bits than vpk_mstep_full" % (im["n"], im["m"], name)
        assert np.array_equal(valid[a:e], (s[a:e] != -1.0).astype(np.int32))
        assert np.array_equal(mx[b], C.max_err_reference(err[a:e]), equal_nan=True)
        worst = max(worst, R.check_mstep(out, im, im["ref"], im["cur"], hard))
    print("mstep %s workgroups %d: worst error / bar %.3g" % ("hard" if hard else "soft", workgroups, worst))
    if hard:
        assert any(((im["assoc"] < 0) | (im["assoc"] >= im["m"])).any() for im in images if _work(im))


@functools.lru_cache(maxsize=None)
def single_positions():
    from vanishing_points_2017_amd import kernels
    return [kernels.mstep(im["l"], im["w"]) if _work(im) else None for im in C.mstep_images(MSTEP_SHAPES, False)]


@pytest.mark.parametrize("workgroups", [0, 2], ids=["grid", "two_workgroups"])
def test_positions_batch(workgroups):
    from vanishing_points_2017_amd import vp_localisation as V
    images = C.mstep_images(MSTEP_SHAPES, False)
    vp, valid = _with(workgroups, 0, lambda: V.calc_new_vanishing_point_batch([im["l"] for im in images], [im["w"] for im in images]))
    vp, valid = _np(vp), _np(valid)
    at = 0
    for im, one in zip(images, single_positions()):
        a, at = at, at + im["m"]
        if not _work(im):
            assert (vp[a:at] == 0).all() and not valid[a:at].any()
            continue
        assert np.array_equal(vp[a:at], one[0], equal_nan=True), (im["n"], im["m"])
        # valid is held to the reference, not to vpk_mstep: that kernel tells a row without a VP by an s it never sets --
        # whatever its LDS held -- while the batch kernel sets it before every image (emstep_device.hpp)
        none = np.array([rec["kind"] == "none" for rec in im["ref"]])
        assert np.array_equal(valid[a:at] == 0, none) and (vp[a:at][none] == 0).all()


# ---- 1 + 2: initial VPs ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single_init(ssize, num_max):
    from vanishing_points_2017_amd import kernels
    return [kernels.init_vps(*R.init_case(ss, nm, kind), num_max=num_max) for ss, nm, kind in R.INIT_CASES if ss == ssize]


@pytest.mark.parametrize("workgroups", [0, 2], ids=["grid", "two_workgroups"])
@pytest.mark.parametrize("ssize", sorted({c[0] for c in R.INIT_CASES}))
def test_init_batch(ssize, workgroups):
    """INIT_CASES grouped by sphere size: every image of a size under every num_max of that size, one launch each."""
    from vanishing_points_2017_amd import vp_localisation as V
    cases = [R.init_case(ss, nm, kind) for ss, nm, kind in R.INIT_CASES if ss == ssize]
    assert len(cases) >= 4
    for num_max in sorted({nm for ss, nm, _ in R.INIT_CASES if ss == ssize}):
        v0, num, wts = _with(workgroups, 0, lambda: V.find_initial_vps_batch([c[1] for c in cases], [c[0] for c in cases], num_max,
                                                                             want_weights=True))
        v0, num, wts = _np(v0), _np(num), _np(wts)
        bare = _with(workgroups, 0, lambda: V.find_initial_vps_batch(np.stack([c[1] for c in cases]), np.stack([c[0] for c in cases]), num_max))
        assert np.array_equal(_np(bare[0]), v0) and np.array_equal(_np(bare[1]), num)      # (weights_out NULL: the same VPs)
        for b, ((cnn, sphere), one) in enumerate(zip(cases, single_init(ssize, num_max))):
            k = int(num[b])
            assert k == one[0].shape[0] and np.array_equal(v0[b, :k], one[0]) and (v0[b, k:] == 0).all()
            assert np.array_equal(wts[b], one[1])
            try:
                want = em.find_initial_vps(sphere, cnn, num_max)
            except ValueError:                                     # np.vstack([]): no cell survives
                want = np.zeros((0, 3))
            assert k == want.shape[0]
            if k:
                assert np.abs(v0[b, :k] - want).max() <= 1e-13
            assert np.array_equal(wts[b], em.pdf_params(cnn.copy()).weights)


# ---- 3: the reference's own intermediates ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stored():
    out = []
    for name in INTERMEDIATES:
        g = load(name)
        assert "i_v0" in g
        g["lnorm"] = g["l"] / np.sqrt((g["l"] ** 2).sum(1))[:, None]
        g["lsim1"] = g["i_lsim"] if "i_lsim" in g else em.calc_lsim(g["lp"], sigma=1)
        out.append(g)
    return out


def test_reference_intermediates():
    from vanishing_points_2017_amd import vp_localisation as V
    gs = stored()
    v0, num = V.find_initial_vps_batch([g["sphere_image"] for g in gs], [g["cnn_response"] for g in gs], 25)
    v0, num = _np(v0), _np(num)
    w = V.weight_matrix_batch([g["i_p_vl0"] for g in gs], [g["i_lweight"] for g in gs], [g["lsim1"] for g in gs], bias=1)
    vp, valid = V.calc_new_vanishing_point_batch([g["lnorm"] for g in gs], [g["i_w0"] for g in gs])
    vp, valid = _np(vp), _np(valid)
    at, rows, left_out, worst = 0, 0, 0, [0.0, 0.0, 0.0]
    for b, g in enumerate(gs):
        m0 = g["i_v0"].shape[0]
        assert num[b] == m0
        worst[0] = max(worst[0], abserr(v0[b, :m0], g["i_v0"]))
        worst[1] = max(worst[1], relerr(_np(w[b]), g["i_w0"]))
        m = g["i_w0"].shape[0]
        assert valid[at:at + m].all()
        for k in range(m):
            rr = g["i_w0"][k] / g["i_w0"][k].max()
            sv = np.linalg.svd(rr[:, None] * g["lnorm"], compute_uv=False)
            rows += 1
            if sv[1] >= 1e-3:
                worst[2] = max(worst[2], abserr(vp[at + k], g["i_mstep0"][k]))
            else:
                left_out += 1
        at += m
    print("initial VPs %.3g (bar 1e-13), weights %.3g relative (bar 1e-10), M-step %.3g (bar 1e-9), %d of %d rows left out by "
          "the rank rule" % (worst[0], worst[1], worst[2], left_out, rows))
    assert worst[0] <= 1e-13 and worst[1] <= 1e-10 and worst[2] <= 1e-9
    assert left_out <= 0.05 * rows


# ---- 4: composition ---------------------------------------------------------------------------------------------------------------
def _chain(measure, host):
    """One iteration from public calls.  host: every stage is fed host copies of the previous stage's output; else every
    intermediate stays a device tensor.  Returns the outputs of every stage, as NumPy."""
    import torch
    from vanishing_points_2017_amd import probability_functions as P
    from vanishing_points_2017_amd import vp_localisation as V
    from vanishing_points_2017_amd.runtime import get_runtime
    dev = get_runtime(0).tdev
    gs = stored()
    maps = np.stack([g["cnn_response"] for g in gs])
    spheres = np.stack([g["sphere_image"] for g in gs])
    lps = [torch.from_numpy(np.ascontiguousarray(g["lp"], dtype=np.float64)).to(dev) for g in gs]
    ls = [torch.from_numpy(np.ascontiguousarray(g["lnorm"])).to(dev) for g in gs]
    off = np.concatenate(([0], np.cumsum([g["lp"].shape[0] for g in gs]))).astype(np.int64)
    pair = (torch.cat(lps), off)

    def hop(x):                                                   # between two stages
        if not host:
            assert all(t.is_cuda for t in (x if isinstance(x, list) else [x]))
            return x
        return [_np(t) for t in x] if isinstance(x, list) else _np(x)

    lsims = V.calc_lsim_batch(pair, sigma=1)
    lscore, langle, llen, off = V.line_geometry_batch(pair, k1=10, k2=4)
    lw = hop(llen * lscore.clamp(0.2, 1))
    v0, num = V.find_initial_vps_batch(spheres, maps, 25)
    vs = hop([v0[b, :k] for b, k in enumerate(num.tolist())])
    ss = [np.full(len(v), (np.pi / (1.282 * 20)) * 1e-6) for v in vs]
    e = P.calc_probabilities_batch(maps, vs, ls, lps, ss, distance_measure=measure)
    p_vl, lvsq = hop([p.vl for p in e['pdf']]), hop([p.lvsq for p in e['pdf']])
    w = hop(V.weight_matrix_batch(p_vl, lw, hop(lsims), bias=1, line_offsets=off))
    r = V.mstep_batch(ls, w, lvsq, p_vl, vs, max_stdd=R.MSTEP_MAX_STDD, s_thresh=R.MSTEP_S_THRESH)
    counts, counts_w, assoc, _, _ = V.calc_vp_line_counts_batch(hop(r['v']), pair[0], hop(r['s']), w, lw, line_offsets=off,
                                                                vp_offsets=r['vp_offsets'])
    flat = lambda x: [np.asarray(t) if host else _np(t) for t in x]
    return {"gs": gs, "vs": flat(vs), "p_vl": flat(p_vl), "lvsq": flat(lvsq), "w": flat(w),
            "out": {k: _np(r[k]) for k in ('v', 's', 'err', 'removed', 'valid', 'max_err')}, "vo": r['vp_offsets'],
            "counts": _np(counts), "counts_w": _np(counts_w), "assoc": _np(assoc)}


@pytest.mark.parametrize("measure", ["angle", "dotprod", "area"])
def test_composed_iteration(measure):
    dev, hst = _chain(measure, False), _chain(measure, True)
    for k in ("vs", "p_vl", "lvsq", "w"):
        for a, b in zip(dev[k], hst[k]):
            assert np.array_equal(a, b, equal_nan=True), k
    for k in dev["out"]:
        assert np.array_equal(dev["out"][k], hst["out"][k], equal_nan=True), k
    for k in ("counts", "counts_w", "assoc"):
        assert np.array_equal(dev[k], hst[k], equal_nan=True), k
    # the NaN pattern mstep_reference predicts, on every image whose inputs are finite
    vo, out, checked = dev["vo"], dev["out"], 0
    for b, g in enumerate(dev["gs"]):
        w, lvsq, p_vl = dev["w"][b], dev["lvsq"][b].T, dev["p_vl"][b]
        if not (np.isfinite(w).all() and np.isfinite(lvsq).all() and np.isfinite(p_vl).all()):
            continue
        checked += 1
        ref = R.mstep_reference(g["lnorm"], w, lvsq, p_vl, None, None, R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH)
        for k, rec in enumerate(ref):
            q = int(vo[b]) + k
            if rec["kind"] == "none":
                assert out["valid"][q] == 0 and out["removed"][q] == 1 and out["s"][q] == -1 and not out["v"][q].any()
            else:
                assert out["valid"][q] == 1 and not np.isnan(out["v"][q]).any()
                assert np.isnan(out["s"][q]) == bool(np.isnan(rec["s"])), (measure, b, k)
                assert not np.isnan(out["err"][q])                                          # (-1 or an angle)
    print("%s: %d of %d images with finite inputs" % (measure, checked, len(dev["gs"])))
    assert checked >= (1 if measure == "angle" else 0)


# ---- 5: the EM's own decision metric ----------------------------------------------------------------------------------------------
def test_consistent_with_the_em():
    import vanishing_points_2017_amd.em as gpu_em
    from vanishing_points_2017_amd import vp_localisation as V
    names = ("yud_n120", "clean3_n60", "tiny_n12")
    gs = [load(n) for n in names]
    res = []
    for g in gs:
        kw = {k: v for k, v in em_kwargs(g).items() if k != "init_vp"}
        assert kw.get("wbias", 1) == 1
        scene = {"l": g["l"].copy(), "lp": g["lp"], "cnn_response": g["cnn_response"], "sphere_image": g["sphere_image"],
                 "init_vp": g.get("init_vp")}
        res.append(gpu_em.em_batch([scene], want_metric=True, want_distribution=True, **kw)[0])
    lps = [g["lp"] for g in gs]
    lsims = V.calc_lsim_batch(lps, sigma=1)
    lscore, langle, llen, off = V.line_geometry_batch(lps, k1=10, k2=4)
    lw = llen * lscore.clamp(0.2, 1)
    w = V.weight_matrix_batch([r["distribution"].vl for r in res], lw, lsims, bias=1, line_offsets=off)
    equal = True
    for b, (name, r) in enumerate(zip(names, res)):
        lwb, lsim, vl = _np(lw[int(off[b]):int(off[b + 1])]), _np(lsims[b]), r["distribution"].vl
        ref, bar = S.smooth_reference(vl * lwb[None, :], 0 * vl, lwb, lsim, 1.0)
        r0 = S.check_smooth(_np(w[b]), ref, bar, "emstep vs EM: batch")
        r1 = S.check_smooth(r["decision_metric"], ref, bar, "emstep vs EM: EM")
        same = np.array_equal(_np(w[b]), r["decision_metric"])
        equal = equal and same
        print("%s: weight_matrix_batch / the EM's decision_metric error over bar %.3g / %.3g, bit-equal: %s" % (name, r0, r1, same))
    print("all three bit-equal: %s" % equal)


# ---- 6: the C-ABI directly ----------------------------------------------------------------------------------------------------------
def test_c_abi_error_cases():
    import torch
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0)
    lib, h, t = rt.lib, rt.h, torch
    OK, ARG, LIMIT = 0, -1, -5                                      # include/vpk.h: VPK_OK, VPK_ERR_ARG, VPK_ERR_LIMIT
    n, m = 6, 2
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    op = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lo, vo, so = i64([0, n]), i64([0, m]), i64([0, n * n])
    dd = lambda k: t.rand(k, dtype=t.float64, device=rt.tdev)
    l, w, lv, p, cur, lw, lsim = dd(3 * n), dd(m * n), dd(m * n), dd(m * n), dd(3 * m), dd(n), dd(n * n)
    assoc = t.zeros(n, dtype=t.int64, device=rt.tdev)
    canary = lambda k, dt=t.float64: t.full((k,), -7, dtype=dt, device=rt.tdev)
    outs = {"vp": canary(3 * 65), "s": canary(65), "err": canary(65), "removed": canary(65, t.int32), "valid": canary(65, t.int32),
            "mx": canary(2), "w": canary(65 * n), "v0": canary(2 * 5 * 3), "m0": canary(2, t.int32), "wts": canary(800, t.float32)}
    P = rt.ptr

    def mstep(batch=1, lo_=lo, vo_=vo, l_=l, w_=w, lv_=lv, p_=p, s_out=outs["s"], err_out=outs["err"], mx=outs["mx"], vp_out=outs["vp"]):
        return lib.vpk_mstep_batch(h, batch, op(lo_), op(vo_), P(l_), P(w_), P(lv_), P(p_), P(assoc), P(cur), 1e-6, 1e-200, P(vp_out),
                                   P(s_out), P(err_out), P(outs["removed"]), P(outs["valid"]), P(mx))

    def weights(batch=1, lo_=lo, vo_=vo, so_=so, p_=p, w_out=outs["w"]):
        return lib.vpk_weight_matrix_batch(h, batch, op(lo_), op(vo_), P(p_), P(lw), op(so_) if so_ is not None else None, P(lsim), 1.0, P(w_out))

    def init(batch=2, cnn=t.zeros(800, dtype=t.float32, device=rt.tdev), sph=t.zeros(2 * 400, dtype=t.uint8, device=rt.tdev), num_max=5, v0=outs["v0"]):
        return lib.vpk_init_vps_batch(h, batch, P(cnn), P(sph), 20, num_max, P(v0), P(outs["m0"]), P(outs["wts"]))

    cases = [
        ("batch = 0", lambda: mstep(batch=0), OK), ("batch = 0", lambda: weights(batch=0), OK), ("batch = 0", lambda: init(batch=0), OK),
        ("batch < 0", lambda: mstep(batch=-1), ARG), ("batch < 0", lambda: weights(batch=-1), ARG), ("batch < 0", lambda: init(batch=-1), ARG),
        ("decreasing offsets", lambda: mstep(batch=2, lo_=i64([0, n, 2]), vo_=i64([0, 1, m])), ARG),
        ("decreasing offsets", lambda: weights(batch=2, lo_=i64([0, 3, n]), vo_=i64([0, m, 1]), so_=i64([0, 9, 18])), ARG),
        ("M = 65", lambda: mstep(vo_=i64([0, 65])), LIMIT), ("M = 65", lambda: weights(vo_=i64([0, 65])), LIMIT),
        ("N = 32769", lambda: mstep(lo_=i64([0, 32769])), LIMIT),
        ("lvsq without p_vl", lambda: mstep(p_=None), ARG), ("p_vl without lvsq", lambda: mstep(lv_=None), ARG),
        ("s_out in positions-only mode", lambda: mstep(lv_=None, p_=None, err_out=None, mx=None), ARG),
        ("max_err_out in positions-only mode", lambda: mstep(lv_=None, p_=None, s_out=None, err_out=None), ARG),
        ("null l", lambda: mstep(l_=None), ARG), ("null vp_out", lambda: mstep(vp_out=None), ARG), ("null s_out", lambda: mstep(s_out=None), ARG),
        ("null p_vl", lambda: weights(p_=None), ARG), ("null w_out", lambda: weights(w_out=None), ARG),
        ("null lsim_offsets", lambda: weights(so_=None), ARG), ("lsim too close", lambda: weights(so_=i64([0, n * n - 1])), ARG),
        ("null cnn", lambda: init(cnn=None), ARG), ("null v0_out", lambda: init(v0=None), ARG),
        ("num_max = 65", lambda: init(num_max=65), ARG), ("num_max = 0", lambda: init(num_max=0), ARG),
    ]
    with rt.on_stream():
        for what, call, want in cases:
            assert call() == want, what
    rt.synchronize()
    for k, o in outs.items():
        assert bool((o == -7).all()), "%s was written by an error case" % k
    # and the calls themselves work on these buffers
    with rt.on_stream():
        assert mstep() == OK and weights() == OK and init() == OK
    rt.synchronize()
    assert not bool((outs["vp"][:3 * m] == -7).any()) and bool((outs["vp"][3 * m:] == -7).all())
    assert not bool((outs["w"][:m * n] == -7).any()) and bool((outs["w"][m * n:] == -7).all())
    assert _np(outs["m0"]).tolist() == [0, 0] and not bool((outs["v0"] == -7).any())         # blank spheres: no VP, zero rows
