"""Float64 restatement of the conv stack's training step, layer by layer, written from the reference's
train/train_val.prototxt:66-288 (Convolution + ReLU, LRN ACROSS_CHANNELS, MAX Pooling) and Caffe's published layer semantics:

    conv   y = relu?(sum_{ic, ky, kx} x[g ICg + ic][oy s - p + ky][ox s - p + kx] w[oc][ic][ky][kx] + b[oc])     (cross-correlation)
           dY' = dY [top > 0];  dW = sum_{b, oy, ox} dY' x;  db = sum dY';  dX = the transposed sum over (oc, ky, kx)
    LRN    s_i = k + (alpha / n) sum_{|j - i| <= n / 2} x_j^2;  y_i = x_i s_i^-beta
           dx_i = dy_i s_i^-beta - (2 alpha beta / n) x_i sum_{|j - i| <= n / 2} dy_j y_j / s_j
    pool   windows [o s, min(o s + K, in)), ceil((in - K) / s) + 1 of them per axis; the maximum is the FIRST element in
           row-major scan order that is strictly greater than all before it; dx = the sum of dy over the windows whose
           maximum the element is
    update V <- mu V + lr_local (dW + decay_local W), W <- W - V                              (train_reference._update)

Layers are plain dicts: {"kind": "conv", "oc", "k", "stride", "pad", "groups", "relu"}, {"kind": "lrn", "n", "alpha", "beta",
"k"}, {"kind": "pool", "k", "stride"}.  The tests feed every function the float32 blobs the layer had ON THE DEVICE (its
input, its output, the gradient that arrived), so each check is local to one layer: a near-tie that a float32 forward decides
differently from a float64 one cannot enter.

With ``bounds=True`` every result comes with a bound on |float32 result - float64 result| that holds for ANY summation order,
with or without fused multiply-adds, under train_reference's rule: a length-K float32 sum of products plus one more add has
error <= (K + 2) u sum|terms|, u = 2^-24.  The inputs of a layer-local check are exact, so no input error is propagated.
    conv forward   K = ICg k k terms and the bias; ReLU passes the error on
    conv dX        K = OCg k k terms; the ReLU's backward is exact (it reads the device's own top)
    conv dW, db    K = B OH OW terms (db: products by 1, exact), whatever the slabs; then _update's five roundings
    pool forward   exact: an equality test.  Pool backward: a sum of at most ceil(K / s)^2 terms
    LRN s          n squares, their sum, the product by alpha / n, the add of k: (n + 3) u (|k| + (alpha / n) sum x^2)
    LRN y          relative: beta e_s / s (the power's condition number) + POW_ULP ulps of powf + one product
    LRN dx         powf and a product; each ratio a product and a quotient; the sum; two products by coef x; the difference
The numbers every element shares -- alpha / n, 2 alpha beta / n, -beta -- are INPUTS, formed in float32 as
csrc/convtrain_device.hpp forms them.  powf on the device is taken as <= POW_ULP ulps (1 ulp <= 2 u relative): ROCm ships no
accuracy table for it, so POW_ULP is the largest error measured on an MI355X over 10^6 arguments s in [1, 4) at
beta = 0.75 (the LRN's range), plus one; see DESIGN 7m."""
import numpy as np
import torch
import torch.nn.functional as F

import train_reference as R

U = R.U
SAFETY = R.SAFETY
POW_ULP = 2.23          # measured 1.2211 ulp on an MI355X, rounded up, plus one


def conv(oc, k, stride=1, pad=0, groups=1, relu=True):
    return dict(kind="conv", oc=oc, k=k, stride=stride, pad=pad, groups=groups, relu=relu)


def lrn(n=5, alpha=1e-4, beta=0.75, k=1.0):
    return dict(kind="lrn", n=n, alpha=alpha, beta=beta, k=k)


def pool(k=3, stride=2):
    return dict(kind="pool", k=k, stride=stride)


EDGE_SHAPE = (1, 47, 39)
EDGE_STACK = [conv(8, 5, stride=2), lrn(), pool(), conv(12, 5, pad=2, groups=2), lrn(), pool(), conv(16, 3, pad=1),
              conv(16, 3, pad=1, groups=2), conv(12, 3, pad=1, groups=2), pool()]
NET_SHAPE = (1, 500, 500)
NET_STACK = [conv(96, 11, stride=4), lrn(), pool(), conv(256, 5, pad=2, groups=2), lrn(), pool(), conv(384, 3, pad=1),
             conv(384, 3, pad=1, groups=2), conv(256, 3, pad=1, groups=2), pool()]       # train_val.prototxt:66-288


def pool_out_size(size, k, stride):
    out = -((k - size) // stride) + 1            # ceil((size - k) / stride) + 1
    return out - 1 if (out - 1) * stride >= size else out        # Caffe: the last window starts inside the plane


def out_shape(shape, d):
    c, h, w = shape
    if d["kind"] == "conv":
        return (d["oc"], (h + 2 * d["pad"] - d["k"]) // d["stride"] + 1, (w + 2 * d["pad"] - d["k"]) // d["stride"] + 1)
    if d["kind"] == "pool":
        return (c, pool_out_size(h, d["k"], d["stride"]), pool_out_size(w, d["k"], d["stride"]))
    return (c, h, w)


def shapes(in_shape, layers):
    out, s = [], tuple(in_shape)
    for d in layers:
        s = out_shape(s, d)
        out.append(s)
    return out


def weight_shapes(in_shape, layers):
    """[(OC, ICg, k, k), (OC,)] per conv layer"""
    out, c = [], in_shape[0]
    for d, s in zip(layers, shapes(in_shape, layers)):
        if d["kind"] == "conv":
            out += [(d["oc"], c // d["groups"], d["k"], d["k"]), (d["oc"],)]
        c = s[0]
    return out


def make_weights(in_shape, layers, seed, momentum=True, gain=1.0):
    """Seeded blobs [W, b, ...] (He-style std, biases 0.1-ish) and momentum blobs of the same shapes"""
    rs = np.random.RandomState(seed)
    w, v = [], []
    for shape in weight_shapes(in_shape, layers):
        if len(shape) == 4:
            fan = shape[1] * shape[2] * shape[3]
            w.append((gain * rs.standard_normal(shape) * np.sqrt(2.0 / fan)).astype(np.float32))
        else:
            w.append((0.1 + 0.05 * rs.standard_normal(shape)).astype(np.float32))
        v.append(((1e-4 * rs.standard_normal(shape)) if momentum else np.zeros(shape)).astype(np.float32))
    return w, v


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _c(count):
    return (count + 2) * U / (1 - (count + 2) * U)


# ---- convolution ---------------------------------------------------------------------------------------------------------
def conv_forward(x, w, b, d, bounds=False):
    kw = dict(stride=d["stride"], padding=d["pad"], groups=d["groups"])
    y = F.conv2d(_t(x), _t(w), _t(b), **kw).numpy()
    if d["relu"]:
        y = np.maximum(y, 0)
    if not bounds:
        return y
    mag = F.conv2d(_t(np.abs(x)), _t(np.abs(w)), _t(np.abs(b)), **kw).numpy()
    terms = w.shape[1] * w.shape[2] * w.shape[3]
    return y, _c(terms) * mag * SAFETY


def conv_backward(x, top, dy, w, d, bounds=False, need_dx=True):
    """(dW, db, dX) of one conv layer from its input x, its OUTPUT top (the ReLU's mask) and the gradient dy that arrived;
    without ``need_dx`` dX and its bound are None"""
    kw = dict(stride=d["stride"], padding=d["pad"], groups=d["groups"])
    x, dy, w = (np.asarray(a, dtype=np.float64) for a in (x, dy, w))
    if d["relu"]:
        dy = np.where(np.asarray(top) > 0, dy, 0.0)
    dw = torch.nn.grad.conv2d_weight(_t(x), w.shape, _t(dy), **kw).numpy()
    db = dy.sum(axis=(0, 2, 3))
    dx = torch.nn.grad.conv2d_input(x.shape, _t(w), _t(dy), **kw).numpy() if need_dx else None
    if not bounds:
        return dw, db, dx
    ady = np.abs(dy)
    red = dy.shape[0] * dy.shape[2] * dy.shape[3]
    edw = _c(red) * torch.nn.grad.conv2d_weight(_t(np.abs(x)), w.shape, _t(ady), **kw).numpy()
    edb = _c(red) * ady.sum(axis=(0, 2, 3))
    terms = (w.shape[0] // d["groups"]) * w.shape[2] * w.shape[3]
    edx = _c(terms) * torch.nn.grad.conv2d_input(x.shape, _t(np.abs(w)), _t(ady), **kw).numpy() * SAFETY if need_dx else None
    return dw, db, dx, edw * SAFETY, edb * SAFETY, edx


def update(w, v, g, eg, lr, decay, mu, bounds=False):
    """train_reference._update: (W', V') and, tracked, their bounds"""
    wn, vn, ew, ev = R._update(np.asarray(w, np.float64), np.asarray(v, np.float64), g, eg, lr, decay, mu, bounds)
    return (wn, vn, ew, ev) if bounds else (wn, vn)


# ---- LRN -----------------------------------------------------------------------------------------------------------------
def lrn_constants(d):
    """(alpha / n, 2 alpha beta / n, beta) as the float32 numbers csrc/convtrain_device.hpp forms, returned as float64"""
    f = np.float32
    aon = f(f(d["alpha"]) / f(d["n"]))
    coef = f(f(f(f(2.0) * f(d["alpha"])) * f(d["beta"])) / f(d["n"]))
    return float(aon), float(coef), float(f(d["beta"]))


def _window_sum(a, n):
    """sum over the channels |j - i| <= n / 2 that exist (axis 1)"""
    h = n // 2
    c = a.shape[1]
    pad = np.zeros(a.shape[:1] + (c + 2 * h,) + a.shape[2:], dtype=a.dtype)
    pad[:, h:h + c] = a
    out = np.zeros_like(a)
    for j in range(n):
        out += pad[:, j:j + c]
    return out


def lrn_forward(x, d, bounds=False):
    """(y, s) and, tracked, (y, s, ey, es)"""
    x = np.asarray(x, dtype=np.float64)
    aon, _, beta = lrn_constants(d)
    kk = float(np.float32(d["k"]))
    sq = aon * _window_sum(x * x, d["n"])
    s = kk + sq
    y = x * s ** -beta
    if not bounds:
        return y, s
    es = (d["n"] + 3) * U * (abs(kk) + sq)
    ey = np.abs(y) * (beta * es / s + POW_ULP * 2 * U + U)
    return y, s, ey * SAFETY, es * SAFETY


def lrn_backward(x, y, s, dy, d, bounds=False):
    """dx from the layer's input x, its output y and scale s (the device's own) and the gradient dy that arrived"""
    x, y, s, dy = (np.asarray(a, dtype=np.float64) for a in (x, y, s, dy))
    _, coef, beta = lrn_constants(d)
    ratio = dy * y / s
    rsum = _window_sum(ratio, d["n"])
    t1, t2 = dy * s ** -beta, coef * x * rsum
    dx = t1 - t2
    if not bounds:
        return dx
    esum = (d["n"] + 2) * U * _window_sum(np.abs(ratio), d["n"])
    edx = np.abs(t1) * (POW_ULP * 2 * U + U) + np.abs(t2) * 2 * U + np.abs(coef * x) * esum + U * np.abs(dx)
    return dx, edx * SAFETY


# ---- MAX pooling ---------------------------------------------------------------------------------------------------------
def pool_forward(x, d):
    """(y, idx): idx the flat index h W + w inside the input plane of the first strict maximum in row-major scan order.
    Exact in any precision: y is a copy."""
    x = np.asarray(x)
    k, st = d["k"], d["stride"]
    b, c, h, w = x.shape
    oh, ow = pool_out_size(h, k, st), pool_out_size(w, k, st)
    ph, pw = (oh - 1) * st + k, (ow - 1) * st + k
    pad = np.full((b, c, ph, pw), -np.inf, dtype=np.float64)
    pad[:, :, :h, :w] = x
    win = np.lib.stride_tricks.sliding_window_view(pad, (k, k), axis=(2, 3))[:, :, ::st, ::st]
    win = win.reshape(b, c, oh, ow, k * k)
    arg = np.argmax(win, axis=-1)                        # NumPy: the first occurrence of the maximum, in window scan order
    ky, kx = arg // k, arg % k
    hh = np.arange(oh)[None, None, :, None] * st + ky
    ww = np.arange(ow)[None, None, None, :] * st + kx
    idx = (hh * w + ww).astype(np.int32)
    y = np.take_along_axis(x.reshape(b, c, h * w), idx.reshape(b, c, -1).astype(np.int64), axis=2).reshape(b, c, oh, ow)
    return y, idx


def pool_backward(dy, idx, in_hw, d, bounds=False):
    dy = np.asarray(dy, dtype=np.float64)
    b, c, oh, ow = dy.shape
    h, w = in_hw
    flat = (np.arange(b * c)[:, None] * (h * w) + idx.reshape(b * c, -1).astype(np.int64)).ravel()
    dx = np.zeros(b * c * h * w)
    np.add.at(dx, flat, dy.ravel())
    dx = dx.reshape(b, c, h, w)
    if not bounds:
        return dx
    mag = np.zeros(b * c * h * w)
    np.add.at(mag, flat, np.abs(dy).ravel())
    per_axis = -(-d["k"] // d["stride"])
    return dx, _c(per_axis * per_axis) * mag.reshape(b, c, h, w) * SAFETY


# ---- the whole stack in float64 (the reference's own consistency, and the learning test) -------------------------------
def stack_forward(x, layers, weights):
    """blobs: per layer a dict with "out" and, by kind, "scale" / "idx".  weights: [W, b, ...] of the conv layers"""
    blobs, cur, wi = [], np.asarray(x, dtype=np.float64), 0
    for d in layers:
        if d["kind"] == "conv":
            o = {"out": conv_forward(cur, weights[wi], weights[wi + 1], d)}
            wi += 2
        elif d["kind"] == "lrn":
            y, s = lrn_forward(cur, d)
            o = {"out": y, "scale": s}
        else:
            y, idx = pool_forward(cur, d)
            o = {"out": y, "idx": idx}
        blobs.append(o)
        cur = o["out"]
    return blobs


def stack_backward(x, layers, weights, blobs, d_top):
    """(weight gradients [dW, db, ...], dX, per-layer gradients with respect to each output) guided by ``blobs``"""
    grads = [None] * len(weights)
    wi = len(weights)
    dy = np.asarray(d_top, dtype=np.float64)
    douts = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        d = layers[l]
        douts[l] = dy
        xin = blobs[l - 1]["out"] if l else np.asarray(x, dtype=np.float64)
        if d["kind"] == "conv":
            wi -= 2
            grads[wi], grads[wi + 1], dy = conv_backward(xin, blobs[l]["out"], dy, weights[wi], d)
        elif d["kind"] == "lrn":
            dy = lrn_backward(xin, blobs[l]["out"], blobs[l]["scale"], dy, d)
        else:
            dy = pool_backward(dy, blobs[l]["idx"], xin.shape[2:], d)
    return grads, dy, douts


def rates(params=None, iteration=0):
    """(lr_w, decay_w, lr_b, decay_b, mu) as the float32 numbers the kernels get"""
    return R.local_rates(dict(R.DEFAULTS, **(params or {})), iteration)[:5]


def head_input_gradient(state, x, t, m6, m7, params=None, iteration=0):
    """(dX, bound) of the dense head's step with respect to its input x: train_reference.step's own backward, continued
    through fc6 with _backward_layer's dx and its bound"""
    params = dict(R.DEFAULTS, **(params or {}))
    dt = np.float64
    st = {k: np.asarray(v, dtype=dt) for k, v in state.items()}
    x, t = np.asarray(x, dtype=dt), np.asarray(t, dtype=dt)
    scale = dt(R.local_rates(params, iteration)[5])
    bsz = x.shape[0]
    f = R._forward(st, x, m6, m7, scale, dt, True)
    out = R._head(f["z"], f["ez"], t, dt(bsz), True)
    dz = (out["sigout"] - t) / dt(bsz)
    edz = (f["ez"] / (4 * bsz) + 6 * U * (1 + np.abs(t)) / bsz) * SAFETY
    _, _, dx, _, _, edx = R._backward_layer(dz, edz, f["d7"], f["ed7"], st["W8"], True)
    da7, eda7 = R._through(dx, edx, f["ms7"], f["y7"], f["ey7"], True)
    _, _, dx, _, _, edx = R._backward_layer(da7, eda7, f["d6"], f["ed6"], st["W7"], True)
    da6, eda6 = R._through(dx, edx, f["ms6"], f["y6"], f["ey6"], True)
    _, _, dx, _, _, edx = R._backward_layer(da6, eda6, x, np.zeros_like(x), st["W6"], True)
    return dx, edx
