"""The dense head's training step on the GPU (vpk_train_*, vanishing_points_2017_amd/train.py) against the float64 NumPy
restatement of the prototxts (tests/train_reference.py), on the same float32 inputs and the same masks.

Single steps are held to the reference's DERIVED bounds (train_reference's docstring: (K + 2) 2^-24 sum|terms| per float32
sum in any order, propagated through the step's later roundings).  The 30-step trajectory is held to a MEASURED one: the
GPU's deviation from the float64 trajectory may be at most 4x that of a plain float32 NumPy run of the same steps (other
summation orders have errors of the same size, not the same errors)."""
import numpy as np
import pytest

import train_reference as R

pytestmark = pytest.mark.gpu

CASES = [((1, 1, 1, 1), 1), ((67, 33, 65, 7), 1), ((67, 33, 65, 7), 5), ((260, 128, 64, 400), 5), ((260, 128, 64, 400), 32),
         ((1027, 19, 4, 3), 17)]
KEYS = ["W6", "b6", "W7", "b7", "W8", "b8"]


def _batch(dims, b, seed):
    """features like pool5 (non-negative, many zeros), labels in [0, 1] (mostly 0/1, some fractional), explicit masks whose
    first row keeps nothing and whose second row keeps everything"""
    rs = np.random.RandomState(seed)
    i, h6, h7, o = dims
    x = np.maximum(rs.standard_normal((b, i)), 0).astype(np.float32)
    t = (rs.random_sample((b, o)) < 0.15).astype(np.float32)
    frac = rs.random_sample((b, o)) < 0.1
    t[frac] = rs.random_sample(int(frac.sum())).astype(np.float32)
    m6 = (rs.random_sample((b, h6)) < 0.5).astype(np.uint8)
    m7 = (rs.random_sample((b, h7)) < 0.5).astype(np.uint8)
    if b >= 2:
        m6[0], m7[0] = 0, 0
        m6[1], m7[1] = 1, 1
    return x, t, m6, m7


def _trainer(dims, state, iteration=0, momentum=True, params=None, seed=0):
    from vanishing_points_2017_amd import train
    tr = train.Head(dims, params=train.SolverParams(**(params or {})), seed=seed)
    tr.load(R.blobs(state))
    if momentum:
        tr.load_momentum(R.blobs(state, "V"))
    tr.iteration = iteration
    return tr


def _read(tr):
    w, v = tr.store(), tr.store_momentum()
    out = dict(zip(KEYS, w))
    out.update({("V" + k) if k[0] == "b" else ("VW" + k[1:]): a for k, a in zip(KEYS, v)})
    return out


@pytest.mark.parametrize("dims,b", CASES)
def test_single_step(dims, b):
    """one step from seeded weights, a nonzero momentum and iteration 200000 (gamma applies once): loss, sigout and every
    W, b and V within the derived bound of the float64 step"""
    state = R.make_state(dims, 100 + b)
    x, t, m6, m7 = _batch(dims, b, 200 + b)
    new, out = R.step(state, x, t, m6, m7, iteration=200000, bounds=True)
    tr = _trainer(dims, state, iteration=200000)
    try:
        loss, sig = tr.step(x, t, masks=(m6, m7))
        loss, sig = float(loss.cpu()), sig.cpu().numpy()
        got = _read(tr)
        assert tr.iteration == 200001
    finally:
        tr.close()
    bnd = out["bounds"]
    print("loss %.9g (float64 %.9g, bound %.3g)" % (loss, out["loss"], bnd["loss"]))
    assert abs(loss - out["loss"]) <= bnd["loss"]
    err = np.abs(sig - out["sigout"])
    print("sigout max err %.3g, max err / bound %.3g" % (err.max(), (err / bnd["sigout"]).max()))
    assert (err <= bnd["sigout"]).all()
    for k in sorted(new):
        err = np.abs(got[k].astype(np.float64) - new[k])
        moved = np.abs(new[k] - state[k].astype(np.float64)).max()
        print("%-4s max err %.3g, max err / bound %.3g, the step moved it by %.3g" % (k, err.max(), (err / bnd[k]).max(), moved))
        assert (err <= bnd[k]).all(), k
        assert moved > 0


def test_generated_masks_are_the_documented_hash():
    """mask = None with a seed equals the step given the masks the host build of the hash makes, bit for bit"""
    from hostsim import simlib_train
    dims, b, seed, it = (67, 33, 65, 7), 5, 1234, 17
    state = R.make_state(dims, 3)
    x, t, _, _ = _batch(dims, b, 4)
    m6 = simlib_train.mask(seed, it, 6, b, dims[1])
    m7 = simlib_train.mask(seed, it, 7, b, dims[2])
    res = []
    for masks in (None, (m6, m7)):
        tr = _trainer(dims, state, iteration=it, seed=seed)
        try:
            loss, sig = tr.step(x, t, masks=masks)
            res.append((loss.cpu().numpy(), sig.cpu().numpy(), _read(tr)))
        finally:
            tr.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    for k in res[0][2]:
        assert np.array_equal(res[0][2][k], res[1][2][k]), k
    assert 0 < m6.sum() < m6.size


def test_two_trainers_give_the_same_bits():
    dims, b = (260, 128, 64, 400), 32
    state = R.make_state(dims, 9)
    batches = [_batch(dims, b, 50 + s) for s in range(3)]
    res = []
    for _ in range(2):
        tr = _trainer(dims, state, seed=77)
        try:
            outs = [tr.step(x, t) for x, t, _, _ in batches]
            res.append(([(l.cpu().numpy(), s.cpu().numpy()) for l, s in outs], _read(tr)))
        finally:
            tr.close()
    for (l0, s0), (l1, s1) in zip(res[0][0], res[1][0]):
        assert np.array_equal(l0, l1) and np.array_equal(s0, s1)
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k]), k
        assert not np.array_equal(res[0][1][k], state[k])


def test_batch_limits():
    from vanishing_points_2017_amd import _lib
    dims = (67, 33, 65, 7)
    state = R.make_state(dims, 1)
    tr = _trainer(dims, state, iteration=5)
    try:
        for b in (0, 33):
            x, t, _, _ = _batch(dims, b, 2)
            with pytest.raises(_lib.VpkError) as ei:
                tr.step(x, t)
            assert "error -5" in str(ei.value) or "error -1" in str(ei.value), str(ei.value)     # VPK_ERR_LIMIT / VPK_ERR_ARG
        tr.synchronize()
        got = _read(tr)
        assert tr.iteration == 5
        for k in got:
            assert np.array_equal(got[k], state[k]), k
    finally:
        tr.close()


def test_refusals():
    """each refusal with its code and with the state unchanged (the head's counterpart of test_gpu_convtrain.py's)"""
    from vanishing_points_2017_amd import _lib, train
    dims = (48, 8, 8, 4)
    state = R.make_state(dims, 5)
    w, v = R.blobs(state), R.blobs(state, "V")
    x, t, m6, m7 = _batch(dims, 2, 6)

    def code(fn, want):
        with pytest.raises(_lib.VpkError) as ei:
            fn()
        assert "error %d" % want in str(ei.value), str(ei.value)

    tr = train.Head(dims)
    try:
        code(tr.store, -4)                                                       # before load
        code(tr.store_momentum, -4)
        code(lambda: tr.load_momentum(v), -4)
        code(lambda: tr.step(x, t), -4)
        code(lambda: tr.evaluate(x, t), -4)
        code(lambda: train.Head(dims, runtime=tr.rt), -4)                        # a second trainer on the handle
        tr.load(w)
        tr.load_momentum(v)
        tr.iteration = 7
        last = train.SolverParams(base_lr=0.01, dropout_ratio=0.25)
        tr.set_params(last)
        code(lambda: setattr(tr, "iteration", -1), -1)
        code(lambda: tr.set_params(train.SolverParams(base_lr=1.0, dropout_ratio=1.0)), -1)
        code(lambda: tr.set_params(train.SolverParams(base_lr=1.0, stepsize=0)), -1)
        rt = tr.rt
        with rt.on_stream():
            dev = [rt.torch.from_numpy(a).to(rt.tdev) for a in (x, t, m6, m7)]
            loss, sig = rt.torch.empty((1,), device=rt.tdev), rt.torch.empty((2, dims[3]), device=rt.tdev)
        for a, b in ((dev[2], None), (None, dev[3])):                            # one mask only
            code(lambda: rt.check(rt.lib.vpk_train_step(rt.h, rt.ptr(dev[0]), rt.ptr(dev[1]), 2, rt.ptr(a), rt.ptr(b), 0, rt.ptr(loss),
                                                        rt.ptr(sig))), -1)
        for b in (0, 33):
            xb, tb, _, _ = _batch(dims, b, 2)
            with pytest.raises(_lib.VpkError) as ei:
                tr.step(xb, tb)
            assert "error -5" in str(ei.value) or "error -1" in str(ei.value), str(ei.value)     # as test_batch_limits
        with pytest.raises(ValueError):
            tr.load(w[:1] + [w[1][:-1]] + w[2:])                                 # a blob of the wrong shape
        with pytest.raises(ValueError):
            tr.load_momentum(v[:5])                                              # ... and a list that is short of one
        tr.synchronize()
        assert tr.iteration == 7 and tr.params is last
        assert all(np.array_equal(p, q) for p, q in zip(tr.store(), w))
        assert all(np.array_equal(p, q) for p, q in zip(tr.store_momentum(), v))
        # the library's own numbers are the ones set last: a step equals, bit for bit, that of a trainer no refusal touched
        twin = _trainer(dims, state, iteration=7, params={"base_lr": 0.01, "dropout_ratio": 0.25})
        try:
            res = []
            for h in (tr, twin):
                loss, sig = h.step(x, t, masks=(m6, m7))
                res.append([loss.cpu().numpy(), sig.cpu().numpy()] + h.store() + h.store_momentum())
            assert all(np.array_equal(p, q) for p, q in zip(*res))
            assert not np.array_equal(res[0][2], w[0]) and tr.iteration == 8
        finally:
            twin.close()
        tr.load(w)
        assert tr.iteration == 0 and all(np.array_equal(p, q) for p, q in zip(tr.store(), w))
        assert all(not m.any() for m in tr.store_momentum())
    finally:
        tr.close()


def test_eval_is_the_forward_without_dropout():
    """B = 70 (three chunks) against the float64 TEST phase; the rows of the first chunk against a step's forward under
    all-one masks with the scale removed (dropout_ratio 0); no weight changes"""
    dims, b = (67, 33, 65, 7), 70
    state = R.make_state(dims, 21)
    x, t, _, _ = _batch(dims, b, 22)
    want = R.evaluate(state, x, t, bounds=True)
    tr = _trainer(dims, state, iteration=3)
    try:
        loss, sig = tr.evaluate(x, t)
        none, sig2 = tr.evaluate(x)
        loss, sig, sig2 = float(loss.cpu()), sig.cpu().numpy(), sig2.cpu().numpy()
        got = _read(tr)
        assert none is None and tr.iteration == 3
    finally:
        tr.close()
    assert np.array_equal(sig, sig2)
    print("loss %.9g (float64 %.9g, bound %.3g)" % (loss, want["loss"], want["bounds"]["loss"]))
    assert abs(loss - want["loss"]) <= want["bounds"]["loss"]
    assert (np.abs(sig - want["sigout"]) <= want["bounds"]["sigout"]).all()
    for k in got:
        assert np.array_equal(got[k], state[k]), k
    st = _trainer(dims, state, params={"dropout_ratio": 0.0})
    try:
        ones = (np.ones((32, dims[1]), np.uint8), np.ones((32, dims[2]), np.uint8))
        _, sig_step = st.step(x[:32], t[:32], masks=ones)
        sig_step = sig_step.cpu().numpy()
    finally:
        st.close()
    assert (np.abs(sig[:32] - sig_step) <= 2 * want["bounds"]["sigout"][:32]).all()


def test_trajectory():
    """30 steps on a fixed batch with fixed masks at base_lr 0.002: the loss falls monotonically after the first few steps
    (first in the float64 reference, which is what admits these inputs), and the final weights stay as close to the float64
    trajectory as a float32 NumPy run does, within a factor 4.  Measured on an MI355X: see DESIGN 7k."""
    dims, b, steps, params = (67, 33, 65, 7), 5, 30, {"base_lr": 0.002}
    state = R.make_state(dims, 31, momentum=False)
    x, t, m6, m7 = _batch(dims, b, 32)
    m6[0], m7[0] = 1, 1                                  # every image takes part
    s64, s32, l64 = state, state, []
    for it in range(steps):
        s64, o = R.step(s64, x, t, m6, m7, params=params, iteration=it)
        s32, _ = R.step(s32, x, t, m6, m7, params=params, iteration=it, dtype=np.float32)
        l64.append(o["loss"])
    assert all(l64[i + 1] < l64[i] for i in range(3, steps - 1)), l64       # the inputs are accepted
    assert l64[-1] < 0.9 * l64[0]
    tr = _trainer(dims, state, momentum=False, params=params)
    try:
        losses = [tr.step(x, t, masks=(m6, m7))[0] for _ in range(steps)]
        losses = [float(v.cpu()) for v in losses]
        got = _read(tr)
    finally:
        tr.close()
    assert all(losses[i + 1] < losses[i] for i in range(3, steps - 1)), losses
    dev_gpu = max(np.abs(got[k].astype(np.float64) - s64[k]).max() for k in KEYS)
    dev_f32 = max(np.abs(s32[k].astype(np.float64) - s64[k]).max() for k in KEYS)
    print("deviation from the float64 trajectory after %d steps: GPU %.3g, float32 NumPy %.3g; loss %.6g -> %.6g" % (
        steps, dev_gpu, dev_f32, losses[0], losses[-1]))
    assert dev_f32 > 0
    assert dev_gpu <= 4 * dev_f32


def test_head_trainer_at_the_net(tmp_path):
    """HeadTrainer at the net's own head (254.4 M parameters, synthetic weights): steps on 5 rasters with label_maps labels,
    then weights() into a fresh cnn.Net gives the response maps evaluate() gives, within the default mode's tolerance against
    float32 (2e-5, tests/test_gpu_cnn.py), and save_caffemodel reads back to the same bytes.  6 s on an MI355X with two steps
    (the synthetic weights, two loads of the net, 1 GB back from the device, 1 GB written and read), so both steps stay."""
    import time
    from vanishing_points_2017_amd import caffe_io, cnn, sphere_mapping, synth, train
    t0 = time.time()
    w, mean = cnn.synthetic_weights(0), cnn.synthetic_mean(0)
    scenes = [synth.make_scene(8100 + i, 120 + 30 * i, 3) for i in range(5)]
    sphere = sphere_mapping.raster_batch([sc["l"] for sc in scenes])
    labels = np.stack([train.label_maps(sc["true_vps"]) for sc in scenes])
    labels[0, 3, 4] = 1.0                                # at least one positive cell whatever the scenes hold
    net = cnn.Net(w, mean)
    tr = train.HeadTrainer(net, w, seed=5)
    try:
        feats = tr.features(sphere)
        assert tuple(feats.shape) == (5, 57600)
        l0, _ = tr.evaluate(feats, labels)
        for _ in range(2):
            loss, sig = tr.step(feats, labels)
        assert tuple(sig.shape) == (5, 400) and np.isfinite(float(loss.cpu()))
        l1, maps = tr.evaluate(sphere, labels)
        maps = maps.cpu().numpy()
        assert float(l1.cpu()) < float(l0.cpu())         # the steps went downhill on their own batch
        w2 = tr.weights()
        path = str(tmp_path / "tuned.caffemodel")
        tr.save_caffemodel(path)
    finally:
        tr.close()
    for name in ("conv1", "conv5"):
        assert w2[name][0] is w[name][0]
    assert not np.array_equal(w2["fc6"][0], w["fc6"][0]) and not np.array_equal(w2["fc8"][1], w["fc8"][1])
    back = caffe_io.read_caffemodel(path)
    for name, _ in cnn.LAYER_SHAPES:
        blobs = back["fc8_20x20" if name == "fc8" else name]
        assert blobs[0].tobytes() == w2[name][0].tobytes() and blobs[1].tobytes() == w2[name][1].tobytes(), name
    got = cnn.Net(w2, mean).forward(sphere)
    assert got.shape == (5, 20, 20)
    print("response maps: max |Net(weights()) - evaluate| %.3g; %.1f s" % (np.abs(got - maps).max(), time.time() - t0))
    assert np.abs(got - maps).max() <= 2e-5

