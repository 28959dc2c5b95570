"""Float64 NumPy restatement of one training step of the dense head, written from the reference's train/train_val.prototxt
(:289-417: fc6, relu6, drop6, fc7, relu7, drop7, fc8_20x20, SigmoidCrossEntropyLoss, sigout) and train/solver.prototxt (SGD,
momentum, weight decay, lr_policy "step"), with Caffe's layer and solver semantics:

    a6 = relu(X W6^T + b6)   d6 = a6 m6 / (1 - p)      a7, d7 likewise      z = d7 W8^T + b8
    loss = sum(max(z, 0) - z t + log1p(exp(-|z|))) / B     sigout = sigmoid(z)     dz = (sigout - t) / B
    dW = dY^T X    db = sum_b dY    dX = dY W, through dropout and ReLU: dA = dX m / (1 - p) [a > 0]     (no dX below fc6)
    V <- mu V + lr_local (dW + decay_local W)     W <- W - V
    lr = base_lr gamma^floor(iter / stepsize); weights lr_mult 1 decay_mult 1, biases lr_mult 2 decay_mult 0

The tests feed it the float32 inputs and masks the GPU gets.  The solver's numbers are INPUTS and are taken as the float32
values the library holds (lr as the float32 product chain); everything downstream of them is float64.

With ``bounds=True`` every output comes with a bound on |float32 result - float64 result| that holds for ANY summation order
and with or without fused multiply-adds.  u = 2^-24.  The rule for a length-K float32 sum of products plus one more add is
    |err| <= (K + 2) u sum|terms|
(each product rounds once, K - 1 additions, one for the bias; first order, made rigorous by the factor 1 / (1 - (K + 2) u)).
An input that itself carries an error e enters with |term| + e |other factor| in the sum and adds e |other factor| outright.
ReLU passes an error on unchanged.  Where the float64 pre-activation lies within its bound of 0 the float32 run may take
the other branch of [a > 0]: there the bound of the back-propagated value is its whole magnitude.  libm calls on the device
(exp, log1p) are taken as <= 2 u relative.  The update's five roundings are added term by term (see ``_update``)."""
import numpy as np

U = 2.0 ** -24
SAFETY = 1.001          # second-order terms of every first-order rule above

DEFAULTS = dict(base_lr=1e-4, gamma=0.1, stepsize=200000, momentum=0.9, weight_decay=5e-4, lr_mult_weight=1.0,
                decay_mult_weight=1.0, lr_mult_bias=2.0, decay_mult_bias=0.0, dropout_ratio=0.5)
LAYERS = ("6", "7", "8")


def learning_rate32(params, iteration):
    """base_lr gamma^floor(iteration / stepsize) as the float32 product chain of csrc/train_device.hpp"""
    lr = np.float32(params["base_lr"])
    for _ in range(int(iteration) // int(params["stepsize"])):
        lr = np.float32(lr * np.float32(params["gamma"]))
    return lr


def local_rates(params, iteration):
    """(lr_w, decay_w, lr_b, decay_b, mu, scale) as the float32 numbers the kernels get, returned as float64"""
    f = np.float32
    lr = learning_rate32(params, iteration)
    lr_w, lr_b = f(lr * f(params["lr_mult_weight"])), f(lr * f(params["lr_mult_bias"]))
    de_w = f(f(params["weight_decay"]) * f(params["decay_mult_weight"]))
    de_b = f(f(params["weight_decay"]) * f(params["decay_mult_bias"]))
    scale = f(f(1.0) / f(f(1.0) - f(params["dropout_ratio"])))
    return tuple(float(v) for v in (lr_w, de_w, lr_b, de_b, f(params["momentum"]), scale))


def make_state(dims, seed, momentum=True, dtype=np.float32):
    """Seeded weights (std 1 / sqrt(fan-in), so that activations stay O(1)), biases 0.1-ish, and a nonzero momentum."""
    rs = np.random.RandomState(seed)
    i, h6, h7, o = dims
    st = {}
    for name, (n, k) in zip(LAYERS, ((h6, i), (h7, h6), (o, h7))):
        st["W" + name] = (rs.standard_normal((n, k)) / np.sqrt(k)).astype(dtype)
        st["b" + name] = (0.1 + 0.05 * rs.standard_normal(n)).astype(dtype)
        st["VW" + name] = ((1e-4 * rs.standard_normal((n, k))) if momentum else np.zeros((n, k))).astype(dtype)
        st["Vb" + name] = ((1e-4 * rs.standard_normal(n)) if momentum else np.zeros(n)).astype(dtype)
    return st


def blobs(state, prefix=""):
    """the six arrays in vpk_train_load's order; prefix "V" for the momentum"""
    out = []
    for name in LAYERS:
        out += [state[("VW" if prefix else "W") + name], state[("Vb" if prefix else "b") + name]]
    return out


def _dense(x, ex, w, b, track):
    y = x @ w.T + b
    if not track:
        return y, None
    k = w.shape[1]
    aw = np.abs(w)
    mag = (np.abs(x) + ex) @ aw.T + np.abs(b)
    ey = (k + 2) * U / (1 - (k + 2) * U) * mag + ex @ aw.T
    return y, ey * SAFETY


def _forward(st, x, m6, m7, scale, dt, track):
    """activations (and their bounds) of the TRAIN phase (masks given) or the TEST phase (masks None)"""
    f = {}
    ex = np.zeros_like(x) if track else None
    y6, e6 = _dense(x, ex, st["W6"], st["b6"], track)
    f["a6"], f["y6"], f["ey6"] = np.maximum(y6, 0), y6, e6
    ms6 = (m6.astype(dt) * dt(scale)) if m6 is not None else np.ones_like(y6)
    f["d6"], f["ms6"] = f["a6"] * ms6, ms6
    ed6 = (ms6 * e6 + U * (np.abs(f["d6"]) + ms6 * e6)) if track else None
    y7, e7 = _dense(f["d6"], ed6, st["W7"], st["b7"], track)
    f["a7"], f["y7"], f["ey7"] = np.maximum(y7, 0), y7, e7
    ms7 = (m7.astype(dt) * dt(scale)) if m7 is not None else np.ones_like(y7)
    f["d7"], f["ms7"] = f["a7"] * ms7, ms7
    ed7 = (ms7 * e7 + U * (np.abs(f["d7"]) + ms7 * e7)) if track else None
    f["ed6"], f["ed7"] = ed6, ed7
    f["z"], f["ez"] = _dense(f["d7"], ed7, st["W8"], st["b8"], track)
    return f


def loss_terms(z, t):
    return np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1 / (1 + e), e / (1 + e))


def _head(z, ez, t, batch_total, track):
    """loss sum / batch_total, sigout and their bounds"""
    out = {}
    terms = loss_terms(z, t) if t is not None else None
    out["sigout"] = sigmoid(z)
    out["loss"] = terms.sum() / batch_total if t is not None else None
    if track:
        out["e_sigout"] = (ez / 4 + 4 * U * out["sigout"]) * SAFETY
        if t is not None:
            n = z.size
            # a term: |d/dz| <= 1; its own roundings: the product, two additions, exp and log1p at 2 u each
            eterm = ez + 6 * U * (np.abs(z) * (1 + np.abs(t)) + np.log1p(np.exp(-np.abs(z))))
            out["e_loss"] = ((eterm.sum() + (n + 2) * U * np.abs(terms).sum()) / batch_total + 2 * U * abs(out["loss"])) * SAFETY
    return out


def _update(w, v, g, eg, lr, decay, mu, track):
    """Caffe's update and, tracked, the bound: t1 = decay w, t2 = g + t1, t3 = lr t2, t4 = mu v, V' = t4 + t3, W' = w - V'"""
    vn = mu * v + lr * (g + decay * w)
    wn = w - vn
    if not track:
        return wn, vn, None, None
    t1 = np.abs(decay * w)
    t2 = np.abs(g) + eg + t1
    ev = lr * eg + U * (lr * t1 + 2 * lr * t2 + np.abs(mu * v) + np.abs(vn) + lr * eg)
    ew = ev + U * (np.abs(wn) + ev)
    return wn, vn, ew * SAFETY, ev * SAFETY


def _backward_layer(dy, edy, x, ex, w, track):
    """dW, db, dX = dY^T X, sum_b dY, dY W with bounds"""
    b, n = dy.shape
    dw, db, dx = dy.T @ x, dy.sum(axis=0), dy @ w
    if not track:
        return dw, db, dx, None, None, None
    ady, ax, aw = np.abs(dy) + edy, np.abs(x) + ex, np.abs(w)
    cb, cn = (b + 2) * U / (1 - (b + 2) * U), (n + 2) * U / (1 - (n + 2) * U)
    edw = cb * (ady.T @ ax) + edy.T @ np.abs(x) + np.abs(dy).T @ ex + edy.T @ ex
    edb = cb * ady.sum(axis=0) + edy.sum(axis=0)
    edx = cn * (ady @ aw) + edy @ aw
    return dw, db, dx, edw * SAFETY, edb * SAFETY, edx * SAFETY


def _through(dx, edx, ms, y, ey, track):
    """dX through dropout and ReLU: dA = dX ms [y > 0]; a pre-activation within its bound of 0 may fall either way"""
    on = y > 0
    g = dx * ms
    da = np.where(on, g, 0)
    if not track:
        return da, None
    eg = ms * edx + U * (np.abs(g) + ms * edx)
    amb = np.abs(y) <= ey
    return da, np.where(amb, np.abs(g) + eg, np.where(on, eg, 0)) * SAFETY


def step(state, x, t, m6, m7, params=None, iteration=0, dtype=np.float64, bounds=False):
    """One solver iteration.  Returns (new_state, out): out has loss, sigout and, tracked, "bounds": {name: bound} for loss,
    sigout and every W, b, VW, Vb.  ``dtype`` float32 gives the plain float32 NumPy run of the trajectory test."""
    params = dict(DEFAULTS, **(params or {}))
    dt = np.dtype(dtype).type
    track = bool(bounds)
    assert not track or dt is np.float64
    st = {k: np.asarray(v, dtype=dt) for k, v in state.items()}
    x, t = np.asarray(x, dtype=dt), np.asarray(t, dtype=dt)
    lr_w, de_w, lr_b, de_b, mu, scale = (dt(v) for v in local_rates(params, iteration))
    bsz = x.shape[0]
    f = _forward(st, x, m6, m7, scale, dt, track)
    out = _head(f["z"], f["ez"], t, dt(bsz), track)
    dz = (out["sigout"] - t) / dt(bsz)
    edz = (f["ez"] / (4 * bsz) + 6 * U * (1 + np.abs(t)) / bsz) * SAFETY if track else None
    new, bnd = {}, {}
    ez0 = np.zeros_like(x) if track else None
    # fc8
    dw, db, dx, edw, edb, edx = _backward_layer(dz, edz, f["d7"], f["ed7"], st["W8"], track)
    new["W8"], new["VW8"], bnd["W8"], bnd["VW8"] = _update(st["W8"], st["VW8"], dw, edw, lr_w, de_w, mu, track)
    new["b8"], new["Vb8"], bnd["b8"], bnd["Vb8"] = _update(st["b8"], st["Vb8"], db, edb, lr_b, de_b, mu, track)
    da7, eda7 = _through(dx, edx, f["ms7"], f["y7"], f["ey7"], track)
    # fc7
    dw, db, dx, edw, edb, edx = _backward_layer(da7, eda7, f["d6"], f["ed6"], st["W7"], track)
    new["W7"], new["VW7"], bnd["W7"], bnd["VW7"] = _update(st["W7"], st["VW7"], dw, edw, lr_w, de_w, mu, track)
    new["b7"], new["Vb7"], bnd["b7"], bnd["Vb7"] = _update(st["b7"], st["Vb7"], db, edb, lr_b, de_b, mu, track)
    da6, eda6 = _through(dx, edx, f["ms6"], f["y6"], f["ey6"], track)
    # fc6: no dX below it
    dw, db, _, edw, edb, _ = _backward_layer(da6, eda6, x, ez0, st["W6"], track)
    new["W6"], new["VW6"], bnd["W6"], bnd["VW6"] = _update(st["W6"], st["VW6"], dw, edw, lr_w, de_w, mu, track)
    new["b6"], new["Vb6"], bnd["b6"], bnd["Vb6"] = _update(st["b6"], st["Vb6"], db, edb, lr_b, de_b, mu, track)
    if track:
        bnd["loss"], bnd["sigout"] = out.pop("e_loss"), out.pop("e_sigout")
        out["bounds"] = bnd
    return new, out


def evaluate(state, x, t=None, bounds=False):
    """The TEST phase: no masks, no scale.  out: loss (None without labels), sigout, and tracked their bounds."""
    dt = np.float64
    st = {k: np.asarray(v, dtype=dt) for k, v in state.items()}
    x = np.asarray(x, dtype=dt)
    t = np.asarray(t, dtype=dt) if t is not None else None
    f = _forward(st, x, None, None, 1.0, dt, bool(bounds))
    out = _head(f["z"], f["ez"], t, dt(x.shape[0]), bool(bounds))
    if bounds:
        out["bounds"] = {"loss": out.pop("e_loss", None), "sigout": out.pop("e_sigout")}
    return out


def mix64(z):
    m = (1 << 64) - 1
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & m
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return z


def mask_bit(seed, iteration, layer, b, j, dropout_ratio=0.5):
    """the keep bit of csrc/train_device.hpp in Python integers (slow: for spot checks of the host build)"""
    m = (1 << 64) - 1
    h0 = mix64((seed + 0x9E3779B97F4A7C15 * (iteration + 1)) & m)
    key = mix64(h0 ^ ((layer << 32) | b))
    thr = int(np.float32(dropout_ratio) * np.float32(16777216.0))
    return 1 if (mix64(key ^ j) >> 40) >= thr else 0
