"""The conv stack's training step on the GPU (vpk_convtrain_*, vpk_train_step_dx; train.ConvStack, train.NetTrainer) against
the float64 restatement of the layers (tests/convtrain_reference.py), LAYER BY LAYER: every layer's input, output, pooling
index, LRN scale and gradient blobs are read back from the device (vpk_convtrain_read) and the layer's forward output, its
data gradient and its updated W, b, VW, Vb are held to the reference's DERIVED bounds computed from the blobs the layer
actually had.  The blobs are shared between neighbouring layers, so this also proves the wiring; a near-tie that float32 and
float64 forwards decide differently cannot enter a check that is local to one layer.  Pooling (values and indices) and the
ReLU's backward are exact: equality tests.  The momentum is nonzero and the iteration is past one learning-rate step."""
import numpy as np
import pytest

import convtrain_reference as C
import train_reference as R

pytestmark = pytest.mark.gpu

ITERATION = 200000           # gamma applies once


def _layer(d):
    from vanishing_points_2017_amd import train
    if d["kind"] == "conv":
        return train.conv_layer(d["oc"], d["k"], d["stride"], d["pad"], d["groups"], d["relu"])
    if d["kind"] == "lrn":
        return train.lrn_layer(d["n"], d["alpha"], d["beta"], d["k"])
    return train.pool_layer(d["k"], d["stride"])


def _stack(in_shape, stack, w=None, v=None, iteration=ITERATION, params=None, runtime=None):
    from vanishing_points_2017_amd import train
    cs = train.ConvStack(in_shape, [_layer(d) for d in stack], params=train.SolverParams(**(params or {})), runtime=runtime)
    if w is not None:
        cs.load(w)
        if v is not None:
            cs.load_momentum(v)
        cs.iteration = iteration
    return cs


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _snapshot(cs, stack, dx=None):
    """every kept blob and the weights, as NumPy arrays"""
    snap = {"out": [], "grad": [], "idx": {}, "scale": {}}
    for l, d in enumerate(stack):
        snap["out"].append(_np(cs.read(l, "output")))
        snap["grad"].append(_np(cs.read(l, "gradient")))
        if d["kind"] == "pool":
            snap["idx"][l] = _np(cs.read(l, "index"))
        if d["kind"] == "lrn":
            snap["scale"][l] = _np(cs.read(l, "scale"))
    snap["w"], snap["v"] = cs.store(), cs.store_momentum()
    snap["dx"] = _np(dx) if dx is not None else None
    return snap


def _same(a, b, skip=()):
    for key in ("out", "grad"):
        for l, (p, q) in enumerate(zip(a[key], b[key])):
            assert np.array_equal(p, q), (key, l)
    for key in ("idx", "scale"):
        for l in a[key]:
            assert np.array_equal(a[key][l], b[key][l]), (key, l)
    for key in ("w", "v"):
        for i, (p, q) in enumerate(zip(a[key], b[key])):
            assert np.array_equal(p, q), (key, i)
    if "dx" not in skip:
        assert np.array_equal(a["dx"], b["dx"])


def _hold(report, name, got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    report[name] = max(report.get(name, 0.0), ratio)
    assert (err <= bound).all(), "%s: largest error / bound %.3g (largest error %.3g)" % (name, ratio, err.max())


def _check_layers(stack, x, w0, v0, snap, params=None, iteration=ITERATION, what=("forward", "dx", "update"), only=None):
    """the layer-local checks; returns {tensor: largest error / bound}"""
    lr_w, de_w, lr_b, de_b, mu = C.rates(params, iteration)
    report, wi = {}, 0
    for l, d in enumerate(stack):
        xin = snap["out"][l - 1] if l else x
        out, dy = snap["out"][l], snap["grad"][l]
        gin = snap["grad"][l - 1] if l else snap["dx"]
        tag = "%d:%s" % (l, d["kind"])
        if d["kind"] == "conv":
            w, b, vw, vb = w0[wi], w0[wi + 1], v0[wi], v0[wi + 1]
            if only is None or l in only:
                if "forward" in what:
                    y, ey = C.conv_forward(xin, w, b, d, bounds=True)
                    _hold(report, tag + " y", out, y, ey)
                need_dx = "dx" in what and gin is not None
                dw, db, dx, edw, edb, edx = C.conv_backward(xin, out, dy, w, d, bounds=True, need_dx=need_dx)
                if need_dx:
                    _hold(report, tag + " dX", gin, dx, edx)
                if "update" in what:
                    wn, vn, ew, ev = C.update(w, vw, dw, edw, lr_w, de_w, mu, bounds=True)
                    _hold(report, tag + " W", snap["w"][wi], wn, ew)
                    _hold(report, tag + " VW", snap["v"][wi], vn, ev)
                    bn, vbn, eb, evb = C.update(b, vb, db, edb, lr_b, de_b, mu, bounds=True)
                    _hold(report, tag + " b", snap["w"][wi + 1], bn, eb)
                    _hold(report, tag + " Vb", snap["v"][wi + 1], vbn, evb)
                    assert np.abs(wn - w).max() > 0 and np.abs(dw).max() > 0, tag
            wi += 2
        elif only is not None and l not in only:
            continue
        elif d["kind"] == "lrn":
            if "forward" in what:
                y, s, ey, es = C.lrn_forward(xin, d, bounds=True)
                _hold(report, tag + " s", snap["scale"][l], s, es)
                _hold(report, tag + " y", out, y, ey)
            if "dx" in what and gin is not None:
                dx, edx = C.lrn_backward(xin, out, snap["scale"][l], dy, d, bounds=True)
                _hold(report, tag + " dX", gin, dx, edx)
        else:
            if "forward" in what:
                y, idx = C.pool_forward(xin, d)
                assert np.array_equal(snap["idx"][l], idx), tag + ": the index is not the first strict maximum of the scan"
                assert np.array_equal(out, y.astype(np.float32)), tag
            if "dx" in what and gin is not None:
                dx, edx = C.pool_backward(dy, snap["idx"][l], xin.shape[2:], d, bounds=True)
                _hold(report, tag + " dX", gin, dx, edx)
    return report


def _run(in_shape, stack, x, d_top, w, v, want_dx=True, params=None):
    cs = _stack(in_shape, stack, w, v, params=params)
    try:
        top = cs.forward(x)
        dx = cs.backward(d_top, want_dx=want_dx)
        snap = _snapshot(cs, stack, dx)
        snap["top"] = _np(top)
        assert cs.iteration == ITERATION + 1
    finally:
        cs.close()
    return snap


def _print(report):
    print("largest error / bound per tensor: " + ", ".join("%s %.3g" % kv for kv in sorted(report.items())))


@pytest.mark.parametrize("batch", [1, 5])
def test_edge_stack(batch):
    """(1, 47, 39): planes 22 x 18 -> 11 x 9 -> 5 x 4 -> 2 x 2, pools with clipped last windows and without, LRN windows cut
    at both channel ends, groups, a strided unpadded first layer"""
    rs = np.random.RandomState(40 + batch)
    x = (2.0 * rs.standard_normal((batch,) + C.EDGE_SHAPE)).astype(np.float32)
    w, v = C.make_weights(C.EDGE_SHAPE, C.EDGE_STACK, 41)
    d_top = rs.standard_normal((batch,) + C.shapes(C.EDGE_SHAPE, C.EDGE_STACK)[-1]).astype(np.float32)
    snap = _run(C.EDGE_SHAPE, C.EDGE_STACK, x, d_top, w, v)
    assert np.array_equal(snap["top"], snap["out"][-1]) and np.array_equal(snap["grad"][-1], d_top)
    report = _check_layers(C.EDGE_STACK, x, w, v, snap)
    _print(report)
    assert np.abs(snap["dx"]).max() > 0


def _tie_planes(rs, shape):
    """planes with exact ties and equal values inside windows, an all-zero plane and a constant negative one"""
    x = rs.randint(-1, 3, size=shape).astype(np.float32)
    x[0, 0] = 0.0
    x[0, 1] = -2.5
    x[-1, -1] = rs.standard_normal(shape[2:]).astype(np.float32)
    return x


ONE_LAYER = {
    "conv_g2": ((20, 37, 29), C.conv(44, 3, pad=1, groups=2), 5),          # nothing a multiple of a tile; 84 slabs, a ragged last
    "conv_s4": ((1, 63, 51), C.conv(10, 11, stride=4), 3),                  # the strided first layer WITH its data gradient
    "conv_lin": ((3, 9, 8), C.conv(5, 2, stride=2, pad=1, relu=False), 2),  # no ReLU, an even kernel
    "lrn7": ((7, 9, 11), C.lrn(), 3),
    "lrn5": ((5, 6, 7), C.lrn(n=5, alpha=0.05, beta=0.75, k=2.0), 2),
    "lrn3_wide": ((70, 5, 9), C.lrn(n=3, alpha=1e-2), 2),                   # more channels than one pass of the channel lanes
    "pool30": ((3, 30, 30), C.pool(), 2),                                   # -> 15, clipped
    "pool61": ((2, 61, 61), C.pool(), 2),                                   # -> 30, exact
}


@pytest.mark.parametrize("name", sorted(ONE_LAYER))
def test_one_layer_stack(name):
    """a one-layer stack with d_input_out is a complete test of the layer"""
    in_shape, d, batch = ONE_LAYER[name]
    rs = np.random.RandomState(len(name) + in_shape[1])
    shape = (batch,) + in_shape
    x = _tie_planes(rs, shape) if d["kind"] == "pool" else (1.5 * rs.standard_normal(shape)).astype(np.float32)
    w, v = C.make_weights(in_shape, [d], 7)
    d_top = rs.standard_normal((batch,) + C.shapes(in_shape, [d])[0]).astype(np.float32)
    if name == "conv_g2":
        from hostsim import simlib_convtrain
        slabs, length = simlib_convtrain.wgrad_slabs(shape, d)
        assert slabs >= 3 and (batch * 37 * 29) % length != 0
    snap = _run(in_shape, [d], x, d_top, w, v)
    report = _check_layers([d], x, w, v, snap)
    _print(report)
    if d["kind"] == "pool":
        win = np.lib.stride_tricks.sliding_window_view(x[:, :, :29, :29], (3, 3), axis=(2, 3))[:, :, ::2, ::2]
        ties = ((win == win.max(axis=(4, 5), keepdims=True)).sum(axis=(4, 5)) > 1).mean()
        assert ties > 0.5                                        # the case is about ties


def _head_batch(dims, b, seed):
    rs = np.random.RandomState(seed)
    i, h6, h7, o = dims
    x = np.maximum(rs.standard_normal((b, i)), 0).astype(np.float32)
    t = (rs.random_sample((b, o)) < 0.15).astype(np.float32)
    m6 = (rs.random_sample((b, h6)) < 0.5).astype(np.uint8)
    m7 = (rs.random_sample((b, h7)) < 0.5).astype(np.uint8)
    return x, t, m6, m7


@pytest.mark.parametrize("batch", [1, 5])
def test_head_dx(batch):
    """vpk_train_step_dx: dX within train_reference._backward_layer's dx bound, and weights, momentum, loss and sigout
    bit-equal to vpk_train_step's"""
    from vanishing_points_2017_amd import train
    dims = (96, 40, 24, 16)
    state = R.make_state(dims, 60 + batch)
    x, t, m6, m7 = _head_batch(dims, batch, 61)
    res = []
    for want_dx in (False, True):
        tr = train.Head(dims, params=train.SolverParams())
        try:
            tr.load(R.blobs(state))
            tr.load_momentum(R.blobs(state, "V"))
            tr.iteration = ITERATION
            out = tr.step(x, t, masks=(m6, m7), want_dx=want_dx)
            res.append(([_np(o) for o in out], tr.store(), tr.store_momentum()))
            assert tr.iteration == ITERATION + 1
        finally:
            tr.close()
    for a, b in zip(res[0][0][:2] + res[0][1] + res[0][2], res[1][0][:2] + res[1][1] + res[1][2]):
        assert np.array_equal(a, b)
    assert not np.array_equal(res[1][1][0], state["W6"])
    want, bound = C.head_input_gradient(state, x, t, m6, m7, iteration=ITERATION)
    report = {}
    _hold(report, "head dX", res[1][0][2], want, bound)
    _print(report)
    assert np.abs(want).max() > 0


def test_composition_and_determinism():
    """the edge stack's blobs and weights equal, bit for bit, the same layers run as one-layer stacks chained by hand on each
    other's device outputs; a second trainer gives the same bits; d_input_out = NULL changes nothing else"""
    batch = 5
    rs = np.random.RandomState(77)
    x = (2.0 * rs.standard_normal((batch,) + C.EDGE_SHAPE)).astype(np.float32)
    w, v = C.make_weights(C.EDGE_SHAPE, C.EDGE_STACK, 78)
    shapes = C.shapes(C.EDGE_SHAPE, C.EDGE_STACK)
    d_top = rs.standard_normal((batch,) + shapes[-1]).astype(np.float32)
    a = _run(C.EDGE_SHAPE, C.EDGE_STACK, x, d_top, w, v)
    b = _run(C.EDGE_SHAPE, C.EDGE_STACK, x, d_top, w, v)
    c = _run(C.EDGE_SHAPE, C.EDGE_STACK, x, d_top, w, v, want_dx=False)
    _same(a, b)
    _same(a, c, skip=("dx",))
    assert c["dx"] is None
    # the chain: every layer a stack of its own
    singles, wi, cur, in_shape = [], 0, x, C.EDGE_SHAPE
    try:
        for l, d in enumerate(C.EDGE_STACK):
            n = 2 if d["kind"] == "conv" else 0
            cs = _stack(in_shape, [d], w[wi:wi + n], v[wi:wi + n])
            singles.append((cs, wi, n))
            wi += n
            cur = cs.forward(cur)
            assert np.array_equal(_np(cur), a["out"][l]), l
            in_shape = shapes[l]
        grad = d_top
        for l in range(len(C.EDGE_STACK) - 1, -1, -1):
            cs, at, n = singles[l]
            assert np.array_equal(_np(grad), a["grad"][l]), l
            grad = cs.backward(grad, want_dx=True)
            got_w, got_v = cs.store(), cs.store_momentum()
            for i in range(n):
                assert np.array_equal(got_w[i], a["w"][at + i]) and np.array_equal(got_v[i], a["v"][at + i]), (l, i)
        assert np.array_equal(_np(grad), a["dx"])
    finally:
        for cs, _, _ in singles:
            cs.close()


def test_refusals():
    """each refusal with its code and with the state unchanged"""
    from vanishing_points_2017_amd import _lib, train
    stack = C.EDGE_STACK[:4]
    w, v = C.make_weights(C.EDGE_SHAPE, stack, 3)
    rs = np.random.RandomState(4)

    def code(fn, want):
        with pytest.raises(_lib.VpkError) as ei:
            fn()
        assert "error %d" % want in str(ei.value), str(ei.value)

    cs = _stack(C.EDGE_SHAPE, stack)
    try:
        x = rs.standard_normal((2,) + C.EDGE_SHAPE).astype(np.float32)
        code(lambda: cs.forward(x), -4)                                          # before load
        code(cs.store, -4)
        code(cs.store_momentum, -4)
        code(lambda: cs.load_momentum(v), -4)
        code(lambda: _stack(C.EDGE_SHAPE, stack, runtime=cs.rt), -4)            # a second trainer on the handle
        cs.load(w)
        cs.load_momentum(v)
        cs.iteration = 7
        top_shape = C.shapes(C.EDGE_SHAPE, stack)[-1]
        code(lambda: cs.backward(np.zeros((0,) + top_shape, np.float32)), -4)   # backward without a forward
        for b in (0, 33):
            code(lambda: cs.forward(np.zeros((b,) + C.EDGE_SHAPE, np.float32)), -5)
        code(lambda: cs.read(0, "output"), -4)                                   # nothing was launched
        top = _np(cs.forward(x))
        code(lambda: cs.read(0, "gradient"), -4)                                 # no backward yet
        code(lambda: cs.read(0, "index"), -1)                                    # layer 0 is no pool
        code(lambda: cs.forward(np.zeros((33,) + C.EDGE_SHAPE, np.float32)), -5)
        assert np.array_equal(_np(cs.read(3, "output")), top)                    # ... and the kept blobs are still there
        cs.backward(np.ones_like(top))
        code(lambda: cs.backward(np.ones_like(top)), -4)                         # a backward consumes its forward
        assert cs.iteration == 8
        cs.load(w)
        assert cs.iteration == 0 and all(np.array_equal(p, q) for p, q in zip(cs.store(), w))
        assert all(not m.any() for m in cs.store_momentum())
    finally:
        cs.close()
    # the head's own trainer lives beside it on the same handle
    head = train.Head((48, 8, 8, 4))
    try:
        both = _stack(C.EDGE_SHAPE, stack, w, v, runtime=head.rt)
        both.close()
    finally:
        head.close()
    bad = [[C.pool(k=3)], [C.conv(4, 7)], [C.conv(4, 3, groups=3)], [C.conv(6, 3, groups=4)], [C.lrn(n=4)],
           [C.conv(4, 3, stride=0)], [C.conv(4, 3, pad=1), C.pool(), C.pool(), C.pool(k=3)]]
    for layers in bad:
        code(lambda: _stack((2, 6, 5) if layers[0].get("groups", 1) > 1 else (1, 2, 6), layers), -1)
    code(lambda: _stack((2, 6, 5), []), -1)
    code(lambda: _stack((513, 2, 2), [C.lrn()]), -5)


def test_stack_trainer_refused_params_change_neither_half():
    """StackTrainer.set_params with numbers the head refuses (dropout_ratio 1) raises and leaves both halves as they were: the
    Python records, and the library's own numbers -- a step equals, bit for bit, that of a trainer that saw no refusal"""
    from vanishing_points_2017_amd import _lib, train
    dims, batch = (48, 32, 32, 16), 2
    rs = np.random.RandomState(60)
    x = (2.0 * rs.standard_normal((batch,) + C.EDGE_SHAPE)).astype(np.float32)
    t = (rs.random_sample((batch, dims[3])) < 0.2).astype(np.float32)
    masks = (np.ones((batch, dims[1]), np.uint8), np.ones((batch, dims[2]), np.uint8))
    w, _ = C.make_weights(C.EDGE_SHAPE, C.EDGE_STACK, 61, momentum=False)
    state = R.make_state(dims, 62, momentum=False)
    res = []
    for refuse in (True, False):
        first = train.SolverParams(base_lr=0.003)
        st = train.StackTrainer(C.EDGE_SHAPE, [_layer(d) for d in C.EDGE_STACK], dims, (w, R.blobs(state)), params=first)
        try:
            if refuse:
                with pytest.raises(_lib.VpkError) as ei:
                    st.set_params(train.SolverParams(base_lr=1.0, dropout_ratio=1.0))
                assert "error -1" in str(ei.value), str(ei.value)
            assert st.stack.params is first and st.head.params is first and st.params is first
            loss, sig = st.step(x, t, masks)
            res.append([_np(loss), _np(sig)] + st.stack.store() + st.head.store())
        finally:
            st.close()
    assert all(np.array_equal(p, q) for p, q in zip(*res))
    assert not np.array_equal(res[0][2], w[0])


class _Net(object):
    """NetTrainer's flow at any geometry: a ConvStack below a Head on one handle"""

    def __init__(self, in_shape, stack, dims, w, state, params):
        from vanishing_points_2017_amd import train
        self.head = train.Head(dims, params=train.SolverParams(**params))
        self.stack = _stack(in_shape, stack, w, None, iteration=0, params=params, runtime=self.head.rt)
        self.head.load(R.blobs(state))

    def step(self, x, t, masks):
        top = self.stack.forward(x)
        loss, sig, dx = self.head.step(top.reshape(top.shape[0], -1), t, masks, want_dx=True)
        self.stack.backward(dx)
        return loss

    def close(self):
        self.stack.close()
        self.head.close()


def _reference_trajectory(in_shape, stack, w, state, x, t, masks, params, steps):
    """the float64 run of the same steps: losses"""
    w = [a.astype(np.float64) for a in w]
    v = [np.zeros_like(a) for a in w]
    losses = []
    for it in range(steps):
        lr_w, de_w, lr_b, de_b, mu = C.rates(params, it)
        blobs = C.stack_forward(x, stack, w)
        feats = blobs[-1]["out"].reshape(x.shape[0], -1)
        dx, _ = C.head_input_gradient(state, feats, t, masks[0], masks[1], params=params, iteration=it)
        state, out = R.step(state, feats, t, masks[0], masks[1], params=params, iteration=it)
        losses.append(out["loss"])
        grads, _, _ = C.stack_backward(x, stack, w, blobs, dx.reshape(blobs[-1]["out"].shape))
        for i, g in enumerate(grads):
            lr, de = (lr_b, de_b) if g.ndim == 1 else (lr_w, de_w)
            w[i], v[i] = C.update(w[i], v[i], g, None, lr, de, mu)
    return losses


def test_learning():
    """twenty whole-net steps of the edge stack under a (48, 32, 32, 16) head on one fixed batch, dropout_ratio 0: the loss
    falls -- first in the float64 reference, which is what admits the seed"""
    dims, batch, steps = (48, 32, 32, 16), 5, 20
    params = {"base_lr": 0.003, "dropout_ratio": 0.0}
    rs = np.random.RandomState(90)
    x = (2.0 * rs.standard_normal((batch,) + C.EDGE_SHAPE)).astype(np.float32)
    t = (rs.random_sample((batch, dims[3])) < 0.2).astype(np.float32)
    masks = (np.ones((batch, dims[1]), np.uint8), np.ones((batch, dims[2]), np.uint8))
    w, _ = C.make_weights(C.EDGE_SHAPE, C.EDGE_STACK, 91, momentum=False)
    state = R.make_state(dims, 92, momentum=False)
    l64 = _reference_trajectory(C.EDGE_SHAPE, C.EDGE_STACK, w, state, x, t, masks, params, steps)
    assert l64[-1] < 0.8 * l64[0] and all(l64[i + 1] < l64[i] for i in range(2, steps - 1)), l64
    net = _Net(C.EDGE_SHAPE, C.EDGE_STACK, dims, w, state, params)
    try:
        losses = [float(net.step(x, t, masks).cpu()) for _ in range(steps)]
        assert net.stack.iteration == net.head.iteration == steps
        w_end = net.stack.store()
    finally:
        net.close()
    print("loss %.6g -> %.6g (float64 %.6g -> %.6g)" % (losses[0], losses[-1], l64[0], l64[-1]))
    assert losses[-1] < 0.8 * losses[0] and all(losses[i + 1] < losses[i] for i in range(2, steps - 1)), losses
    assert all(not np.array_equal(p, q) for p, q in zip(w_end, w))           # the conv stack moved, every blob of it


def test_net_geometry(tmp_path):
    """NetTrainer at the net's own stack, B = 2, seeded sparse rasters, cnn.synthetic_weights:
    (a) the stack's forward blobs at the eight conv-stack taps against the float64 net (oracle/cnn_torch.py) at the project's
        bar for f32 kernels, 2e-4 (1 + max|ref|) (tests/test_gpu_cnn.py), and pool5's indices bit-equal to the scan rule;
    (b) the layer-local check of conv1-conv5's updates after one NetTrainer.step with given masks;
    (c) save_caffemodel -> caffe_io -> cnn.Net: the stored conv blobs are the trainer's."""
    from oracle import cnn_torch
    from vanishing_points_2017_amd import caffe_io, cnn, sphere_mapping, synth, train
    w, mean = cnn.synthetic_weights(0), cnn.synthetic_mean(0)
    scenes = [synth.make_scene(8200 + i, 140 + 40 * i, 3) for i in range(2)]
    sphere = sphere_mapping.raster_batch([sc["l"] for sc in scenes])
    labels = np.stack([train.label_maps(sc["true_vps"]) for sc in scenes])
    labels[0, 3, 4] = 1.0
    rs = np.random.RandomState(5)
    masks = ((rs.random_sample((2, 4096)) < 0.5).astype(np.uint8), (rs.random_sample((2, 4096)) < 0.5).astype(np.uint8))
    _, taps = cnn_torch.forward(w, mean, sphere, want_taps=True, dtype=np.float64)
    nt = train.NetTrainer(w, mean, seed=3)
    try:
        w0 = nt.stack.store()
        v0 = [(1e-4 * rs.standard_normal(a.shape)).astype(np.float32) for a in w0]
        nt.stack.load_momentum(v0)
        nt.iteration = ITERATION
        x = _np(nt._data(sphere))
        loss, sig = nt.step(sphere, labels, masks=masks)
        assert nt.iteration == ITERATION + 1 and tuple(sig.shape) == (2, 400) and np.isfinite(float(loss.cpu()))
        stack = C.NET_STACK
        snap = _snapshot(nt.stack, stack)
        for tap, l in enumerate([0, 2, 3, 5, 6, 7, 8, 9]):
            want = taps[cnn_torch.TAPS[tap]]
            err = np.abs(snap["out"][l] - want).max()
            assert err <= 2e-4 * (1.0 + np.abs(want).max()), (cnn_torch.TAPS[tap], err)
        _, idx = C.pool_forward(snap["out"][8], stack[9])
        assert np.array_equal(snap["idx"][9], idx)
        report = _check_layers(stack, x, w0, v0, snap, iteration=ITERATION, what=("update",))
        _print(report)
        w2 = nt.weights()
        path = str(tmp_path / "net.caffemodel")
        nt.save_caffemodel(path)
    finally:
        nt.close()
    for k, name in enumerate(train.CONV_LAYERS):
        assert np.array_equal(w2[name][0], snap["w"][2 * k]) and not np.array_equal(w2[name][0], w[name][0]), name
    back = caffe_io.read_caffemodel(path)
    for name, _ in cnn.LAYER_SHAPES:
        blobs = back["fc8_20x20" if name == "fc8" else name]
        assert blobs[0].tobytes() == w2[name][0].tobytes() and blobs[1].tobytes() == w2[name][1].tobytes(), name
    got = cnn.Net({n: (back["fc8_20x20" if n == "fc8" else n][0], back["fc8_20x20" if n == "fc8" else n][1])
                   for n, _ in cnn.LAYER_SHAPES}, mean).forward(sphere)
    assert got.shape == (2, 20, 20) and np.isfinite(got).all()
