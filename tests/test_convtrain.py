"""The conv stack's training step without a GPU: the host build of csrc/convtrain_device.hpp (tests/hostsim/sim_convtrain.cpp)
against the float64 reference (tests/convtrain_reference.py) per element -- pooling windows and output sizes, the scan-order
argmax with ties, the LRN of short channel columns, the convolution's three index maps against torch's own float64
gradients -- the net's exported descriptor, the C-ABI, and the reference's own consistency with torch autograd."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convtrain_reference as C
from conftest import ROOT
from hostsim import simlib_convtrain as S

POOLS = [(3, 2), (2, 2), (3, 1), (3, 3), (5, 2), (2, 3)]


def _ratio(got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    tiny = np.finfo(np.float64).tiny
    return float((err / np.maximum(bound, tiny)).max()) if err.size else 0.0


def test_pool_sizes_and_windows():
    """every (size, K, stride), size 3..62: Caffe's ceil-mode count, windows that start inside the plane, end at its edge and
    are never empty, and the inverse map (the windows that contain an element) against brute force"""
    for k, stride in POOLS:
        for size in range(max(3, k), 63):
            out = S.pool_out_size(size, k, stride)
            ceil = -((k - size) // stride) + 1
            assert out == C.pool_out_size(size, k, stride) == (ceil - 1 if (ceil - 1) * stride >= size else ceil)
            assert out == ceil or k < stride
            wins = [S.pool_window(o, k, stride, size) for o in range(out)]
            for o, (lo, hi) in enumerate(wins):
                assert lo == o * stride and hi == min(lo + k, size) and lo < hi <= size
            if k >= stride:
                assert wins[-1][1] == size                       # the plane is covered to its edge
                clipped = wins[-1][1] - wins[-1][0] < k
                assert clipped == ((size - k) % stride != 0)
            for i in range(size):
                lo, hi = S.pool_windows_of(i, k, stride, out)
                assert [o for o in range(out) if wins[o][0] <= i < wins[o][1]] == list(range(lo, hi + 1)), (size, k, stride, i)
    assert S.pool_out_size(2, 3, 2) == 0                         # a pool larger than its plane does not chain
    assert S.pool_out_size(61, 3, 2) == 30 and S.pool_out_size(30, 3, 2) == 15 and S.pool_out_size(123, 3, 2) == 61


def _scan_argmax(plane, h0, h1, w0, w1):
    best, m = None, None
    for h in range(h0, h1):
        for w in range(w0, w1):
            if best is None or plane[h, w] > m:
                best, m = h * plane.shape[1] + w, plane[h, w]
    return best


@pytest.mark.parametrize("size,k,stride", [(30, 3, 2), (13, 3, 2), (9, 2, 2), (11, 5, 2), (7, 3, 1)])
def test_pool_argmax_with_ties(size, k, stride):
    """planes of few distinct values (ties in nearly every window), an all-zero plane and a constant one: the index is the
    first strict maximum of the row-major scan, in the host build, in the reference and by the rule written out"""
    rs = np.random.RandomState(size)
    x = rs.randint(0, 3, size=(6, size, size + 1)).astype(np.float32)
    x[0] = 0.0
    x[1] = -2.5
    y, idx = S.pool_forward(x, k, stride)
    ry, ridx = C.pool_forward(x[None], dict(k=k, stride=stride))
    assert np.array_equal(idx, ridx[0]) and np.array_equal(y, ry[0].astype(np.float32))
    ties = 0
    for p in range(x.shape[0]):
        for oh in range(idx.shape[1]):
            for ow in range(idx.shape[2]):
                h0, h1 = S.pool_window(oh, k, stride, size)
                w0, w1 = S.pool_window(ow, k, stride, size + 1)
                assert idx[p, oh, ow] == _scan_argmax(x[p], h0, h1, w0, w1)
                ties += int((x[p, h0:h1, w0:w1] == y[p, oh, ow]).sum() > 1)
    assert ties > idx.size // 2                                  # the case is about ties
    dy = rs.standard_normal(y.shape).astype(np.float32)
    dx = S.pool_backward(dy, idx, x.shape[1:], k, stride)
    want, bound = C.pool_backward(dy[None], ridx, x.shape[1:], dict(k=k, stride=stride), bounds=True)
    assert (np.abs(dx - want[0]) <= bound[0]).all()
    assert np.abs(dx).sum() > 0 and (dx[0].reshape(-1)[np.setdiff1d(np.arange(x[0].size), idx[0].ravel())] == 0).all()


@pytest.mark.parametrize("n", [1, 3, 5, 7])
def test_lrn_on_short_channel_columns(n):
    """columns of 1..9 channels, so that windows are cut at one end, at both, or not at all; large and tiny values"""
    rs = np.random.RandomState(n)
    d = C.lrn(n=n, alpha=1e-4 if n != 3 else 0.5, beta=0.75, k=1.0 if n != 7 else 2.0)
    worst = {"s": 0.0, "y": 0.0, "dx": 0.0}
    for c in range(1, 10):
        for scale in (1e-3, 1.0, 300.0):
            x = (scale * rs.standard_normal(c)).astype(np.float32)
            dy = rs.standard_normal(c).astype(np.float32)
            s, y = S.lrn_forward(x, n, d["alpha"], d["beta"], d["k"])
            ry, rs_, ey, es = C.lrn_forward(x.reshape(1, c, 1, 1), d, bounds=True)
            worst["s"] = max(worst["s"], _ratio(s, rs_.ravel(), es.ravel()))
            worst["y"] = max(worst["y"], _ratio(y, ry.ravel(), ey.ravel()))
            dx = S.lrn_backward(x, y, s, dy, n, d["alpha"], d["beta"])
            rdx, edx = C.lrn_backward(*(a.reshape(1, c, 1, 1) for a in (x, y, s, dy)), d, bounds=True)
            worst["dx"] = max(worst["dx"], _ratio(dx, rdx.ravel(), edx.ravel()))
    print("largest error / bound:", worst)
    assert max(worst.values()) <= 1.0, worst
    # the formula itself: autograd of torch's own LRN in float64
    x = torch.from_numpy(rs.standard_normal((2, 7, 3, 2))).requires_grad_()
    y = F.local_response_norm(x, n, alpha=C.lrn_constants(d)[0] * n, beta=d["beta"], k=d["k"])
    dy = torch.from_numpy(rs.standard_normal(y.shape))
    y.backward(dy)
    ry, rscale = C.lrn_forward(x.detach().numpy(), d)
    assert np.allclose(ry, y.detach().numpy(), rtol=1e-12, atol=0)
    _, coef, _ = C.lrn_constants(d)
    want = x.grad.numpy()
    got = C.lrn_backward(x.detach().numpy(), ry, rscale, dy.numpy(), d)
    # the reference's coefficient is the float32 2 alpha beta / n: compare at that coefficient's own rounding
    assert np.allclose(got, want, rtol=0, atol=4 * C.U * np.abs(want).max() + 1e-12)


CONVS = [((2, 1, 23, 19), C.conv(6, 5, stride=2, pad=0)),
         ((3, 6, 9, 11), C.conv(8, 3, pad=1, groups=2)),
         ((2, 4, 12, 10), C.conv(6, 3, stride=3, pad=2, groups=2, relu=False)),
         ((5, 2, 17, 16), C.conv(3, 4, stride=1, pad=0))]


@pytest.mark.parametrize("xshape,d", CONVS)
def test_conv_index_maps_against_torch(xshape, d):
    """forward, data gradient and weight gradient through gemm_a / gemm_b / gemm_store on the host against torch's float64
    conv2d and ITS gradients (torch.nn.grad), within the derived bounds: strides, padding, groups, ragged slabs"""
    rs = np.random.RandomState(sum(xshape))
    x = rs.standard_normal(xshape).astype(np.float32)
    (ws, bs) = C.weight_shapes(xshape[1:], [d])
    w, b = rs.standard_normal(ws).astype(np.float32), rs.standard_normal(bs).astype(np.float32)
    y = S.conv_forward(x, w, b, d)
    ry, ey = C.conv_forward(x, w, b, d, bounds=True)
    assert y.shape == ry.shape and (np.abs(y - ry) <= ey).all(), _ratio(y, ry, ey)
    if d["relu"]:
        assert 0 < (y > 0).mean() < 1
    dy = rs.standard_normal(y.shape).astype(np.float32)
    dw, db, dx, edw, edb, edx = C.conv_backward(x, y, dy, w, d, bounds=True)
    # torch autograd agrees with torch.nn.grad on the same masked gradient
    xt, wt = torch.from_numpy(x.astype(np.float64)).requires_grad_(), torch.from_numpy(w.astype(np.float64)).requires_grad_()
    yt = F.conv2d(xt, wt, torch.from_numpy(b.astype(np.float64)), stride=d["stride"], padding=d["pad"], groups=d["groups"])
    mask = torch.from_numpy((y > 0).astype(np.float64)) if d["relu"] else torch.ones_like(yt)
    yt.backward(torch.from_numpy(dy.astype(np.float64)) * mask)
    assert np.allclose(dx, xt.grad.numpy(), rtol=1e-12, atol=1e-13) and np.allclose(dw, wt.grad.numpy(), rtol=1e-12, atol=1e-13)
    got_dx = S.conv_dgrad(xshape, w, y, dy, d)
    assert (np.abs(got_dx - dx) <= edx).all(), _ratio(got_dx, dx, edx)
    got_dw, got_db, slabs = S.conv_wgrad(x, y, dy, d)
    assert (np.abs(got_dw - dw) <= edw).all(), _ratio(got_dw, dw, edw)
    assert (np.abs(got_db - db) <= edb).all(), _ratio(got_db, db, edb)
    assert np.abs(dx).max() > 0 and np.abs(dw).max() > 0


def test_weight_gradient_slabs():
    """the split depends on the geometry and B alone, covers the reduction in whole chunks, and the one-layer GPU case
    (conv 20 -> 44 k3 p1 g2 on 37 x 29 at B = 5) spans at least three slabs with a ragged last one"""
    d = C.conv(44, 3, pad=1, groups=2)
    slabs, length = S.wgrad_slabs((5, 20, 37, 29), d)
    red = 5 * 37 * 29
    assert slabs >= 3 and length % S.CHUNK == 0 and (slabs - 1) * length < red <= slabs * length and red % length != 0
    for shape, dd in [((5, 1, 500, 500), C.NET_STACK[0]), ((32, 96, 61, 61), C.NET_STACK[3]), ((1, 256, 30, 30), C.NET_STACK[6]),
                      ((1, 1, 5, 5), C.conv(1, 5))]:
        slabs, length = S.wgrad_slabs(shape, dd)
        oh = S.conv_out_size(shape[2], dd["k"], dd["stride"], dd["pad"])
        red = shape[0] * oh * oh
        assert slabs >= 1 and length % S.CHUNK == 0 and (slabs - 1) * length < red <= slabs * length


def _built():
    from vanishing_points_2017_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("libvpk.so not built (run python -m vanishing_points_2017_amd.build)")
    return _lib


def test_net_descriptor():
    """vpk_convtrain_net_layers against the prototxt's numbers as the reference file states them, and its shapes against
    cnn.TAP_SHAPES / cnn.LAYER_SHAPES"""
    _lib = _built()
    from vanishing_points_2017_amd import cnn, train
    shape, layers = train.net_stack()
    assert shape == C.NET_SHAPE and len(layers) == len(C.NET_STACK) == 10
    kinds = {"conv": _lib.LAYER_CONV, "lrn": _lib.LAYER_LRN, "pool": _lib.LAYER_POOL}
    for got, want in zip(layers, C.NET_STACK):
        assert got.kind == kinds[want["kind"]]
        if want["kind"] == "conv":
            assert (got.out_channels, got.kernel, got.stride, got.pad, got.groups, got.relu) == (
                want["oc"], want["k"], want["stride"], want["pad"], want["groups"], 1)
        elif want["kind"] == "lrn":
            assert got.local_size == want["n"]
            assert (got.alpha, got.beta, got.k) == tuple(float(np.float32(want[f])) for f in ("alpha", "beta", "k"))
        else:
            assert (got.kernel, got.stride) == (want["k"], want["stride"])
    shapes = train.stack_shapes(shape, layers)
    assert shapes == C.shapes(C.NET_SHAPE, C.NET_STACK)
    taps = [0, 2, 3, 5, 6, 7, 8, 9]                      # conv1, pool1, conv2, pool2, conv3, conv4, conv5, pool5
    assert [shapes[i] for i in taps] == cnn.TAP_SHAPES[:8]
    assert C.weight_shapes(C.NET_SHAPE, C.NET_STACK)[0::2] == [s for _, s in cnn.LAYER_SHAPES[:5]]
    assert int(np.prod(shapes[-1])) == train.NET_DIMS[0]
    # the Python size rules are the library's
    for size in range(3, 63):
        assert train.stack_shapes((1, size, size), [train.pool_layer(3, 2)])[0][1] == S.pool_out_size(size, 3, 2)
        assert train.stack_shapes((1, size, size), [train.conv_layer(1, 3, stride=2, pad=1)])[0][1] == S.conv_out_size(size, 3, 2, 1)


def test_abi_names_and_argtypes():
    _lib = _built()
    names = ["vpk_convtrain_net_layers", "vpk_convtrain_create", "vpk_convtrain_destroy", "vpk_convtrain_set_params",
             "vpk_convtrain_load", "vpk_convtrain_store", "vpk_convtrain_load_momentum", "vpk_convtrain_store_momentum",
             "vpk_convtrain_set_iteration", "vpk_convtrain_get_iteration", "vpk_convtrain_forward", "vpk_convtrain_backward",
             "vpk_convtrain_read", "vpk_train_step_dx"]
    header = open(os.path.join(ROOT, "include", "vpk.h")).read()
    lib = _lib.load()
    for n in names:
        assert n in _lib.EXPORTS, n
        assert re.search(r"\bint %s\s*\(" % n, header), n
        assert getattr(lib, n).argtypes is not None, n
    assert lib.vpk_train_step_dx.argtypes == lib.vpk_train_step.argtypes + [ctypes.c_void_p]
    assert len(lib.vpk_convtrain_create.argtypes) == 6 and len(lib.vpk_convtrain_read.argtypes) == 4
    units = __import__("vanishing_points_2017_amd.build", fromlist=["UNITS"]).UNITS
    assert "vpk_convtrain.hip" in units
    assert lib.vpk_version() == 110
    # the descriptor struct is the header's: eleven 4-byte fields
    assert ctypes.sizeof(_lib.StackLayer) == 44
    m = re.search(r"typedef struct vpk_stack_layer \{(.*?)\} vpk_stack_layer;", header, re.S)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", m.group(1))
    assert fields == [n for n, _ in _lib.StackLayer._fields_]


def _torch_stack(x, layers, weights):
    cur, wi = x, 0
    for d in layers:
        if d["kind"] == "conv":
            cur = F.conv2d(cur, weights[wi], weights[wi + 1], stride=d["stride"], padding=d["pad"], groups=d["groups"])
            cur = F.relu(cur) if d["relu"] else cur
            wi += 2
        elif d["kind"] == "lrn":
            cur = F.local_response_norm(cur, d["n"], alpha=C.lrn_constants(d)[0] * d["n"], beta=d["beta"], k=d["k"])
        else:
            cur = F.max_pool2d(cur, d["k"], d["stride"], ceil_mode=True)
    return cur


def test_reference_backward_is_autograd_on_the_edge_stack():
    """the reference's guided float64 backward of the edge stack equals torch autograd in float64.  Ties are absent here by
    construction of the inputs: that is asserted on every pooling window, not assumed"""
    rs = np.random.RandomState(5)
    x = rs.standard_normal((3,) + C.EDGE_SHAPE)
    w, _ = C.make_weights(C.EDGE_SHAPE, C.EDGE_STACK, 6)
    w = [a.astype(np.float64) for a in w]
    blobs = C.stack_forward(x, C.EDGE_STACK, w)
    assert [b["out"].shape[1:] for b in blobs] == C.shapes(C.EDGE_SHAPE, C.EDGE_STACK)
    assert [s[1:] for s in C.shapes(C.EDGE_SHAPE, C.EDGE_STACK)][0::1][0] == (22, 18)
    assert [C.shapes(C.EDGE_SHAPE, C.EDGE_STACK)[i][1:] for i in (2, 5, 9)] == [(11, 9), (5, 4), (2, 2)]
    for l, d in enumerate(C.EDGE_STACK):
        if d["kind"] != "pool":
            continue
        xin = blobs[l - 1]["out"]
        out = blobs[l]["out"]
        for oh in range(out.shape[2]):
            for ow in range(out.shape[3]):
                win = xin[:, :, oh * 2:oh * 2 + 3, ow * 2:ow * 2 + 3]
                hits = (win == out[:, :, oh:oh + 1, ow:ow + 1]).sum(axis=(2, 3))
                assert (hits[out[:, :, oh, ow] != 0] == 1).all(), (l, oh, ow)      # (a window of zeros passes no gradient on: relu)
    d_top = rs.standard_normal(blobs[-1]["out"].shape)
    grads, dx, _ = C.stack_backward(x, C.EDGE_STACK, w, blobs, d_top)
    xt = torch.from_numpy(x).requires_grad_()
    wt = [torch.from_numpy(a).requires_grad_() for a in w]
    top = _torch_stack(xt, C.EDGE_STACK, wt)
    assert np.allclose(top.detach().numpy(), blobs[-1]["out"], rtol=1e-12, atol=1e-14)
    top.backward(torch.from_numpy(d_top))
    # the LRN's backward coefficient is the float32 2 alpha beta / n: relative 2^-24 on that term
    for got, want in zip(grads + [dx], [t.grad.numpy() for t in wt] + [xt.grad.numpy()]):
        assert np.abs(want).max() > 0
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
