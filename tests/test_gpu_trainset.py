"""The device-resident training set, the trainers' state and the solver's loop on the GPU (vpk_trainset_*; train.TrainSet,
train.StackTrainer, train.Solver) against tests/trainset_reference.py: equalities for the gathered and transformed lines,
VPs, cells and label maps, for the rasters of the composition, for the mean image, and bit-for-bit comparisons of every
loop the solver runs with the same loop written out by hand."""
import ctypes

import numpy as np
import pytest

import convtrain_reference as C
import train_reference as R
import trainset_reference as T

pytestmark = pytest.mark.gpu

SMALL = 40                                                   # the raster size of the small geometry
SMALL_SHAPE = (1, SMALL, SMALL)
SMALL_STACK = [C.conv(8, 5, stride=2), C.pool(), C.conv(16, 3, pad=1, groups=2), C.pool()]   # 18 -> 9 -> 9 -> 4
SMALL_DIMS = (16 * 4 * 4, 32, 32, 16)
SMALL_GRID = (4, 4)
LEARN_LR = 0.003     # admitted by the float64 trajectory below (test_learning): its test loss falls at this rate
_cache = {}


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _layers():
    from vanishing_points_2017_amd import train
    out = []
    for d in SMALL_STACK:
        out.append(train.conv_layer(d["oc"], d["k"], d["stride"], d["pad"], d["groups"], d["relu"]) if d["kind"] == "conv"
                   else train.pool_layer(d["k"], d["stride"]))
    return out


def _edge():
    if "edge" not in _cache:
        _cache["edge"] = T.edge_set()
    return _cache["edge"]


def _set(size=SMALL, grid=(20, 20)):
    """one TrainSet per (size, grid) of the ten-image set, shared and never changed"""
    from vanishing_points_2017_amd import train
    key = ("set", size, grid)
    if key not in _cache:
        lines, vps = _edge()
        _cache[key] = train.TrainSet(lines, vps, size=size, grid=grid)
    return _cache[key]


def _augment():
    from vanishing_points_2017_amd import train
    return train.Augment(*T.EDGE_AUGMENT)


def _mean():
    if "mean" not in _cache:
        _cache["mean"] = _set(SMALL, SMALL_GRID).mean_image(chunk=3)
    return _cache["mean"]


def _small_weights(seed=70):
    w, _ = C.make_weights(SMALL_SHAPE, SMALL_STACK, seed, momentum=False)
    state = R.make_state(SMALL_DIMS, seed + 1, momentum=False)
    return w, state


def _trainer(params=None, seed=5, weight_seed=70):
    from vanishing_points_2017_amd import train
    w, state = _small_weights(weight_seed)
    return train.StackTrainer(SMALL_SHAPE, _layers(), SMALL_DIMS, (w, R.blobs(state)), mean=_mean(),
                              params=train.SolverParams(**(params or {})), seed=seed)


def _state_equal(a, b):
    assert a["iteration"] == b["iteration"] and a["seed"] == b["seed"]
    for name in ("conv_weights", "conv_momentum", "head_weights", "head_momentum"):
        assert len(a[name]) == len(b[name]) and len(a[name]) > 0
        for k, (p, q) in enumerate(zip(a[name], b[name])):
            assert p.dtype == q.dtype == np.float32 and p.shape == q.shape, (name, k)
            assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), (name, k)       # the bits, without a copy


# ---- vpk_trainset_batch against the reference ---------------------------------------------------------------------------------
def _compare_parts(parts, lines, vps, grid, identity):
    want = T.batch(lines, vps, parts["index"].tolist(), parts["transforms"], grid)
    assert np.array_equal(parts["offsets"], want["offsets"])
    for g in T.EDGE_GRIDS:                                   # the condition on the inputs, for every VP
        assert T.margin(want["vp_out"], g) >= T.MARGIN
    assert _np(parts["l_out"]).tobytes() == want["l_out"].tobytes()
    assert _np(parts["vp_out"]).tobytes() == want["vp_out"].tobytes()
    assert np.array_equal(_np(parts["cell_out"]), want["cell_out"])
    labels = _np(parts["labels"])
    assert labels.dtype == np.float32 and labels.tobytes() == want["labels"].tobytes()
    if identity:
        assert parts["transforms"] is None
        assert _np(parts["l_out"]).tobytes() == np.concatenate([lines[i] for i in parts["index"]], 0).tobytes()
    return want


@pytest.mark.parametrize("batch,iteration", T.edge_cases())
def test_batch_parts(batch, iteration):
    lines, vps = _edge()
    for grid in T.EDGE_GRIDS:
        ts = _set(SMALL, grid)
        parts = ts.batch_parts(iteration or 0, batch, seed=0, augment=None if iteration is None else _augment())
        assert parts["index"].tolist() == T.indices(iteration or 0, batch, 10, 0, False)
        if iteration is not None:
            assert np.array_equal(parts["transforms"], T.augment_transforms(0, iteration, batch, *T.EDGE_AUGMENT))
        want = _compare_parts(parts, lines, vps, grid, iteration is None)
        assert tuple(parts["rasters"].shape) == (batch, SMALL, SMALL) and tuple(parts["labels"].shape) == (batch, grid[0] * grid[1])
    if batch == 32:
        assert len(set(parts["index"].tolist())) < batch                      # repeats
        assert (want["cell_out"] == -1).sum() >= 3 and (want["labels"].sum(1) == 0).any()


def test_batch_parts_repeated_index_and_explicit_identity():
    lines, vps = _edge()
    ts = _set(SMALL, (20, 20))
    index = np.array([3, 3, 0, 5, 3, 6, 0], dtype=np.int32)
    h = _augment().transforms(4, 2, index.shape[0])
    _compare_parts(ts.batch_parts(0, index.shape[0], indices=index, transforms=h), lines, vps, (20, 20), False)
    _compare_parts(ts.batch_parts(0, index.shape[0], indices=index), lines, vps, (20, 20), True)
    from vanishing_points_2017_amd import train
    parts = ts.batch_parts(0, 4, indices=index[:4], augment=train.Augment())       # the default Augment is the copy too
    _compare_parts(parts, lines, vps, (20, 20), True)
    only_empty = ts.batch_parts(0, 2, indices=np.array([0, 0], dtype=np.int32), augment=_augment())
    assert tuple(only_empty["l_out"].shape) == (0, 3) and not _np(only_empty["labels"]).any()
    assert np.array_equal(_np(only_empty["rasters"][0]), _np(only_empty["rasters"][1]))


@pytest.mark.parametrize("size", [SMALL, 500])
def test_composition(size):
    """batch = gather + transform + vpk_sphere_raster: the rasters are raster_batch's of the reference's transformed lines"""
    from vanishing_points_2017_amd import sphere_mapping
    lines, vps = _edge()
    ts = _set(size, (20, 20))
    aug = _augment()
    for iteration, batch in ((0, 5), (1, 5)) if size == 500 else ((0, 5), (1, 5), (6, 32)):
        rasters, labels = ts.batch(iteration, batch, seed=0, augment=aug, check=True)
        index = T.indices(iteration, batch, 10, 0, False)
        want = T.batch(lines, vps, index, T.augment_transforms(0, iteration, batch, *T.EDGE_AUGMENT), (20, 20))
        ref = sphere_mapping.raster_batch(want["lines"], size=size)
        assert _np(rasters).tobytes() == ref.tobytes(), (size, iteration)
        assert _np(labels).tobytes() == want["labels"].tobytes()
        if iteration == 0:                                   # image 0 has no line: the frame-only canvas
            frame = sphere_mapping.raster_batch([np.zeros((0, 3))], size=size)[0]
            assert np.array_equal(_np(rasters[0]), frame) and not np.array_equal(_np(rasters[2]), frame)


def _raw(ts, index, transforms, out_offsets, gh, gw, outs, batch=None):
    rt = ts.rt
    vp = ctypes.c_void_p
    index = np.ascontiguousarray(index, dtype=np.int32)
    out_offsets = np.ascontiguousarray(out_offsets, dtype=np.int64)
    if transforms is not None:
        transforms = np.ascontiguousarray(transforms, dtype=np.float64)
    with rt.on_stream():
        return rt.lib.vpk_trainset_batch(
            rt.h, rt.ptr(ts.l), ts.line_offsets.ctypes.data_as(vp), rt.ptr(ts.vps), ts.vp_offsets.ctypes.data_as(vp), ts.n,
            index.ctypes.data_as(vp), transforms.ctypes.data_as(vp) if transforms is not None else None,
            index.shape[0] if batch is None else batch, out_offsets.ctypes.data_as(vp), gh, gw, *[rt.ptr(o) for o in outs])


def test_refusals():
    import torch
    ts = _set(SMALL, (20, 20))
    rt = ts.rt
    good_index = np.array([2, 4, 2], dtype=np.int32)
    counts = np.array([T.EDGE_LINES[i] for i in good_index])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ident = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (3, 1))
    with rt.on_stream():
        outs = [torch.full((int(off[-1]), 3), 7.0, dtype=torch.float64, device=rt.tdev),
                torch.full((8, 3), 7.0, dtype=torch.float64, device=rt.tdev),
                torch.full((8,), 7, dtype=torch.int32, device=rt.tdev),
                torch.full((3, 400), 7.0, dtype=torch.float32, device=rt.tdev)]
    singular, nan, inf = ident.copy(), ident.copy(), ident.copy()
    singular[1] = (1.0, 2.0, 0.0, 2.0, 4.0, 0.0)
    nan[2, 5] = np.nan
    inf[0, 0] = np.inf
    bad_off = off.copy()
    bad_off[1] += 1
    cases = {"index n": (np.array([2, 10, 2]), ident, off, 20, 20, None), "index -1": (np.array([2, -1, 2]), ident, off, 20, 20, None),
             "offsets": (good_index, ident, bad_off, 20, 20, None), "offsets start": (good_index, ident, off + 1, 20, 20, None),
             "det == 0": (good_index, singular, off, 20, 20, None), "NaN": (good_index, nan, off, 20, 20, None),
             "inf": (good_index, inf, off, 20, 20, None), "gw = 65": (good_index, None, off, 20, 65, None),
             "gh = 0": (good_index, None, off, 0, 20, None), "B = 0": (good_index, None, off, 20, 20, 0)}
    for name, (index, h, o, gh, gw, batch) in cases.items():
        assert _raw(ts, index, h, o, gh, gw, outs, batch) == -1, name
        assert name and rt.lib.vpk_last_error(rt.h)
    assert rt.lib.vpk_trainset_batch(None, *([None] * 4), 1, None, None, 1, None, 20, 20, *([None] * 4)) == -1
    rt.synchronize()
    for o in outs:
        assert (_np(o) == 7).all()                            # nothing was launched
    assert _raw(ts, good_index, ident, off, 20, 20, outs) == 0        # ... and the same buffers are written by a good call
    rt.synchronize()
    assert not (_np(outs[0]) == 7).any() and _np(outs[3]).max() == 1.0
    # the Python layer passes the refusal on
    from vanishing_points_2017_amd import _lib
    with pytest.raises(_lib.VpkError) as ei:
        ts.batch_parts(0, 2, indices=np.array([0, 10], dtype=np.int32))
    assert "error -1" in str(ei.value)
    with pytest.raises(_lib.VpkError) as ei:
        ts.batch_parts(0, 2, transforms=np.zeros((2, 6)))
    assert "error -1" in str(ei.value)


def test_mean_image(tmp_path):
    import torch
    from vanishing_points_2017_amd import caffe_io, sphere_mapping, train
    lines, _ = _edge()
    rasters = sphere_mapping.raster_batch(lines, size=SMALL)
    want = rasters.astype(np.float64).mean(0).astype(np.float32)
    got = _mean()                                             # chunks of 3: 3 + 3 + 3 + 1
    assert got.dtype == np.float32 and got.shape == (SMALL, SMALL) and got.tobytes() == want.tobytes()
    assert got.min() < got.max()
    ts = _set(SMALL, SMALL_GRID)
    path = str(tmp_path / "mean.binaryproto")
    ts.save_mean(path)
    back = caffe_io.read_binaryproto(path)
    assert back.shape == (1, 1, SMALL, SMALL) and back.tobytes() == want.tobytes()
    # the uint32 sums refuse the image that could overflow them
    rt = ts.rt
    with rt.on_stream():
        r = torch.full((2, 16), 255, dtype=torch.uint8, device=rt.tdev)
        total = torch.full((16,), 9, dtype=torch.int32, device=rt.tdev)
    count = ctypes.c_int64(train.MAX_MEAN_IMAGES - 1)
    assert rt.lib.vpk_trainset_accumulate(rt.h, rt.ptr(r), 2, 16, rt.ptr(total), ctypes.byref(count)) == -5
    assert count.value == train.MAX_MEAN_IMAGES - 1
    for bad in ((0, 16, 0), (1, 0, 0), (1, 16, -1)):
        c = ctypes.c_int64(bad[2])
        assert rt.lib.vpk_trainset_accumulate(rt.h, rt.ptr(r), bad[0], bad[1], rt.ptr(total), ctypes.byref(c)) == -1
    rt.synchronize()
    assert (_np(total) == 9).all()
    assert rt.lib.vpk_trainset_accumulate(rt.h, rt.ptr(r), 1, 16, rt.ptr(total), ctypes.byref(count)) == 0
    assert count.value == train.MAX_MEAN_IMAGES
    count = ctypes.c_int64(0)
    assert rt.lib.vpk_trainset_accumulate(rt.h, rt.ptr(r), 2, 16, rt.ptr(total), ctypes.byref(count)) == 0
    rt.synchronize()
    assert (_np(total) == 9 + 3 * 255).all() and count.value == 2


def test_determinism():
    from vanishing_points_2017_amd import runtime, train
    lines, vps = _edge()
    a = _set(SMALL, SMALL_GRID)
    b = train.TrainSet(lines, vps, size=SMALL, grid=SMALL_GRID, runtime=runtime.Runtime(0))      # a handle of its own
    aug = _augment()
    first = [_np(x) for x in a.batch(3, 5, seed=2, augment=aug, shuffle=True)]
    other = [_np(x) for x in b.batch(3, 5, seed=2, augment=aug, shuffle=True)]
    assert all(p.tobytes() == q.tobytes() for p, q in zip(first, other))
    assert a.indices(3, 5, 2, True).tolist() == T.indices(3, 5, 10, 2, True)
    for t in (0, 7, 4):                                       # batch(t) does not depend on the calls before it
        a.batch(t, 32, seed=9, augment=aug)
    again = [_np(x) for x in a.batch(3, 5, seed=2, augment=aug, shuffle=True)]
    assert all(p.tobytes() == q.tobytes() for p, q in zip(first, again))
    assert not np.array_equal(first[0], _np(a.batch(3, 5, seed=3, augment=aug, shuffle=True)[0]))
    b.rt.handle.close()


# ---- the solver against the loop written out by hand --------------------------------------------------------------------------
SOLVER_KW = dict(batch_size=5, shuffle=True, seed=21, log=None)


def _straight_six():
    """six iterations of Solver.step on the small geometry, dropout on, augmented and shuffled: the state they end in"""
    from vanishing_points_2017_amd import train
    if "six" not in _cache:
        ts = _set(SMALL, SMALL_GRID)
        tr = _trainer()
        try:
            sv = train.Solver(tr, ts, augment=_augment(), **SOLVER_KW)
            losses = _np(sv.step(6))
            assert losses.shape == (6,) and np.isfinite(losses).all() and tr.iteration == 6
            _cache["six"] = (tr.state(), losses)
        finally:
            tr.close()
    return _cache["six"]


def test_solver_equals_manual_loop():
    from vanishing_points_2017_amd import train
    want, want_losses = _straight_six()
    ts = _set(SMALL, SMALL_GRID)
    aug = _augment()
    w, state = _small_weights()
    assert all(not np.array_equal(p, q) for p, q in zip(want["conv_weights"], w))                 # it trained, every blob
    assert all(m.any() for m in want["conv_momentum"] + want["head_momentum"])
    # (a) StackTrainer driven by hand
    tr = _trainer()
    try:
        losses = []
        for t in range(6):
            rasters, labels = ts.batch(t, 5, seed=21, augment=aug, shuffle=True)
            losses.append(float(tr.step(rasters, labels)[0]))
        _state_equal(tr.state(), want)
        assert np.array_equal(np.array(losses, dtype=np.float32), want_losses)
    finally:
        tr.close()
    # (b) the ConvStack + Head pair driven by hand
    params = train.SolverParams()
    head = train.Head(SMALL_DIMS, params=params, seed=5)
    stack = train.ConvStack(SMALL_SHAPE, _layers(), params=params, runtime=head.rt)
    try:
        stack.load(w)
        head.load(R.blobs(state))
        mean = head.rt.torch.from_numpy(_mean()).to(head.rt.tdev)
        for t in range(6):
            rasters, labels = ts.batch(t, 5, seed=21, augment=aug, shuffle=True)
            x = (rasters.to(head.rt.torch.float32) - mean).reshape(5, 1, SMALL, SMALL)
            top = stack.forward(x)
            _, _, dx = head.step(top.reshape(5, -1), labels, None, want_dx=True)
            stack.backward(dx)
        pair = {"iteration": head.iteration, "seed": head.seed, "conv_weights": stack.store(), "conv_momentum": stack.store_momentum(),
                "head_weights": head.store(), "head_momentum": head.store_momentum()}
        assert stack.iteration == 6
        _state_equal(pair, want)
    finally:
        stack.close()
        head.close()


def test_resume(tmp_path):
    """three iterations, a snapshot, a fresh trainer and solver, restore, three more = six straight"""
    from vanishing_points_2017_amd import train
    want, _ = _straight_six()
    ts = _set(SMALL, SMALL_GRID)
    prefix = str(tmp_path / "small")
    tr = _trainer()
    try:
        sv = train.Solver(tr, ts, augment=_augment(), snapshot_prefix=prefix, **SOLVER_KW)
        sv.step(3)
        path = sv.snapshot()
        assert path == prefix + "_iter_3.solverstate.npz"
    finally:
        tr.close()
    tr = _trainer(seed=999, weight_seed=123)                  # other weights and another dropout seed: the snapshot's must win
    try:
        sv = train.Solver(tr, ts, augment=_augment(), **dict(SOLVER_KW, seed=0))
        saved = sv.restore(path)
        assert tr.iteration == 3 and sv.seed == 21 and saved["shuffle"] is True and saved["augment"]["mirror"] == 0.5
        sv.step(3)
        _state_equal(tr.state(), want)
    finally:
        tr.close()


def test_test_phase():
    from vanishing_points_2017_amd import train
    ts = _set(SMALL, SMALL_GRID)
    tr = _trainer()
    try:
        sv = train.Solver(tr, ts, test_set=ts, test_batch=70, test_iter=3, **SOLVER_KW)
        sv.step(2)
        before = tr.state()
        got = sv.test()
        manual = []
        for k in range(3):
            rasters, labels = ts.batch(k, 70)
            assert rasters.shape[0] == 70                     # past the 32-row chunks of the evaluation
            manual.append(float(tr.evaluate(rasters, labels)[0]))
        assert got == float(np.mean(np.array(manual, dtype=np.float64)))
        _state_equal(tr.state(), before)
    finally:
        tr.close()


def reference_learning(rasters_of, labels_of, mean, lr, steps, batch=5, n=10):
    """the float64 run (convtrain_reference + train_reference) of ``steps`` solver iterations on the batches of Caffe's
    cursor, dropout off: the test loss (two batches of five from the set's start) before and after"""
    params = {"base_lr": lr, "dropout_ratio": 0.0}
    w, state = _small_weights()
    w = [a.astype(np.float64) for a in w]
    v = [np.zeros_like(a) for a in w]
    ones = (np.ones((batch, SMALL_DIMS[1]), np.uint8), np.ones((batch, SMALL_DIMS[2]), np.uint8))

    def data(t):
        x = rasters_of(t).astype(np.float64) - mean.astype(np.float64)
        return x.reshape(batch, 1, SMALL, SMALL), labels_of(t).astype(np.float64)

    def test_loss():
        out = []
        for k in range(n // batch):
            x, t = data(k)
            feats = C.stack_forward(x, SMALL_STACK, w)[-1]["out"].reshape(batch, -1)
            out.append(R.evaluate(state, feats, t)["loss"])
        return float(np.mean(out))

    first = test_loss()
    for it in range(steps):
        x, t = data(it)
        lr_w, de_w, lr_b, de_b, mu = C.rates(params, it)
        blobs = C.stack_forward(x, SMALL_STACK, w)
        feats = blobs[-1]["out"].reshape(batch, -1)
        dx, _ = C.head_input_gradient(state, feats, t, ones[0], ones[1], params=params, iteration=it)
        state, _ = R.step(state, feats, t, ones[0], ones[1], params=params, iteration=it)
        grads, _, _ = C.stack_backward(x, SMALL_STACK, w, blobs, dx.reshape(blobs[-1]["out"].shape))
        for i, g in enumerate(grads):
            rate, de = (lr_b, de_b) if g.ndim == 1 else (lr_w, de_w)
            w[i], v[i] = C.update(w[i], v[i], g, None, rate, de, mu)
    return first, test_loss()


def test_learning():
    """thirty iterations at base_lr = LEARN_LR on the ten-image set, dropout off, no augmentation: the test loss on the
    training set falls -- first in the float64 reference, which is what admits the rate.  The run is bit-reproducible
    (test_solver_equals_manual_loop), so the result cannot flicker."""
    from vanishing_points_2017_amd import train
    lines, vps = _edge()
    ts = _set(SMALL, SMALL_GRID)
    batches = {}

    def parts(t):
        if t % 2 not in batches:                              # ten images in fives: two distinct batches
            r, l = ts.batch(t % 2, 5)
            batches[t % 2] = (_np(r), _np(l))
        return batches[t % 2]

    f0, f1 = reference_learning(lambda t: parts(t)[0], lambda t: parts(t)[1], _mean(), LEARN_LR, 30)
    assert f1 < 0.9 * f0, (f0, f1)
    tr = _trainer(params={"base_lr": LEARN_LR, "dropout_ratio": 0.0})
    try:
        sv = train.Solver(tr, ts, test_set=ts, batch_size=5, test_batch=5, test_iter=2, log=None)
        g0 = sv.test()
        sv.step(30)
        g1 = sv.test()
    finally:
        tr.close()
    print("test loss %.6g -> %.6g (float64 %.6g -> %.6g)" % (g0, g1, f0, f1))
    assert g1 < g0
    # the same net on both sides: float32 sums of at most 258 products through four layers stay far inside 1e-4 relative
    assert abs(g0 - f0) <= 1e-4 * f0


def test_net_geometry(tmp_path):
    """NetTrainer under the solver at the net's own sizes: two iterations at B = 2 on four synthetic scenes equal the manual
    loop bit for bit, and the snapshot's caffemodel reads back to weights()' bytes"""
    from vanishing_points_2017_amd import caffe_io, cnn, synth, train
    w, mean = cnn.synthetic_weights(0), cnn.synthetic_mean(0)
    scenes = [synth.make_scene(8300 + i, 120 + 30 * i, 3) for i in range(4)]
    ts = train.TrainSet.from_scenes(scenes, size=500)
    assert len(ts) == 4 and ts.grid == (20, 20)
    prefix = str(tmp_path / "net")
    states = []
    for manual in (False, True):
        nt = train.NetTrainer(w, mean, seed=3)
        try:
            if manual:
                for t in range(2):
                    rasters, labels = ts.batch(t, 2, seed=1, shuffle=True)
                    nt.step(rasters, labels)
            else:
                sv = train.Solver(nt, ts, batch_size=2, shuffle=True, seed=1, snapshot_prefix=prefix, log=None)
                sv.step(2)
                sv.snapshot()
                w2 = nt.weights()
            states.append(nt.state())
        finally:
            nt.close()
    _state_equal(states[0], states[1])
    assert states[0]["iteration"] == 2 and not np.array_equal(states[0]["conv_weights"][0], w["conv1"][0])
    back = caffe_io.read_caffemodel(prefix + "_iter_2.caffemodel")
    for name, _ in cnn.LAYER_SHAPES:
        blobs = back["fc8_20x20" if name == "fc8" else name]
        assert blobs[0].tobytes() == w2[name][0].tobytes() and blobs[1].tobytes() == w2[name][1].tobytes(), name
    with np.load(prefix + "_iter_2.solverstate.npz") as z:
        assert int(z["iteration"]) == 2 and z["head_weights_0"].tobytes() == w2["fc6"][0].tobytes()
    labels = _np(ts.batch(0, 4)[1]).reshape(4, 20, 20)
    for k, sc in enumerate(scenes):
        assert T.margin(sc["true_vps"], (20, 20)) >= T.MARGIN
        assert np.array_equal(labels[k], train.label_maps(sc["true_vps"]))
