"""Fine-tuning the net's dense head (fc6, fc7, fc8) on the GPU: the reference's train/train_val.prototxt:289-417 under
train/solver.prototxt, without Caffe (C-ABI: vpk_train_*, csrc/vpk_train.hip).

The conv stack stays frozen: ``HeadTrainer.features`` takes pool5 from the forward (``Net.forward_device(sphere, tap=7)``)
and a step trains the three InnerProduct layers on it -- 254.4 M of the net's 258 M parameters.  ``Head`` is the C-ABI at
any layer sizes; ``HeadTrainer`` is ``Head`` at the net's sizes next to a ``cnn.Net``.  There is no CPU fallback."""
import ctypes

import numpy as np

from . import _lib, caffe_io, cnn, coordinate_conversion
from .runtime import Runtime

HEAD_LAYERS = ("fc6", "fc7", "fc8")
NET_DIMS = (57600, 4096, 4096, 400)      # pool5 = cnn.TAP_SHAPES[7] flattened, fc6, fc7, fc8_20x20
MAX_BATCH = 32                           # rows of one vpk_train_step


class SolverParams(object):
    """The solver's numbers with the prototxts' defaults (solver.prototxt:8-18; train_val.prototxt:294-301, 326)."""

    FIELDS = tuple(n for n, _ in _lib.TrainParams._fields_)

    def __init__(self, base_lr=1e-4, gamma=0.1, stepsize=200000, momentum=0.9, weight_decay=5e-4, lr_mult_weight=1.0,
                 decay_mult_weight=1.0, lr_mult_bias=2.0, decay_mult_bias=0.0, dropout_ratio=0.5):
        self.base_lr = float(base_lr)
        self.gamma = float(gamma)
        self.stepsize = int(stepsize)
        self.momentum = float(momentum)
        self.weight_decay = float(weight_decay)
        self.lr_mult_weight = float(lr_mult_weight)
        self.decay_mult_weight = float(decay_mult_weight)
        self.lr_mult_bias = float(lr_mult_bias)
        self.decay_mult_bias = float(decay_mult_bias)
        self.dropout_ratio = float(dropout_ratio)

    def as_dict(self):
        return {n: getattr(self, n) for n in self.FIELDS}

    def as_struct(self):
        p = _lib.TrainParams()
        for n in self.FIELDS:
            setattr(p, n, getattr(self, n))
        return p

    @classmethod
    def library_defaults(cls):
        """What vpk_train_default_params sets (needs libvpk.so, no GPU)."""
        p = _lib.TrainParams()
        _lib.load().vpk_train_default_params(ctypes.byref(p))
        return cls(**{n: getattr(p, n) for n in cls.FIELDS})

    def learning_rate(self, iteration):
        """lr_policy "step" (solver.prototxt:9): base_lr * gamma^floor(iteration / stepsize)."""
        return self.base_lr * self.gamma ** (int(iteration) // self.stepsize)


def label_maps(vps_or_angles, shape=(20, 20)):
    """The label of one image: a float32 ``shape`` map with 1 in the cell of every ground-truth vanishing point.

    ``vps_or_angles``: (n, 3) vectors in the normalised frame (any length, either sign) or (n, 2) angles (alpha, beta).  The
    cell is the nearest one to ``coordinate_conversion.angle_to_index(point_to_angle(vp), shape)``, i.e. the cell whose
    ``index_to_angle`` the response map is read with.  VPs outside the map are dropped; two VPs in one cell give one 1."""
    arr = np.asarray(vps_or_angles, dtype=np.float64)
    out = np.zeros(shape, dtype=np.float32)
    if arr.size == 0:
        return out
    if arr.ndim == 1:
        arr = arr[None]
    if arr.ndim != 2 or arr.shape[1] not in (2, 3):
        raise ValueError("label_maps takes (n, 3) vanishing points or (n, 2) angles, got shape %s" % (arr.shape,))
    for row in arr:
        if arr.shape[1] == 3:
            norm = np.sqrt(np.sum(row * row))
            if not norm > 0 or not np.all(np.isfinite(row)):
                continue
            p = row / norm
            if p[2] < 0:
                p = -p
            angle = coordinate_conversion.point_to_angle(p)
        else:
            angle = row
        idx = coordinate_conversion.angle_to_index(angle, shape)
        if not np.all(np.isfinite(idx)):
            continue
        a, b = int(np.floor(idx[0] + 0.5)), int(np.floor(idx[1] + 0.5))
        if 0 <= a < shape[0] and 0 <= b < shape[1]:
            out[a, b] = 1.0
    return out


class Head(object):
    """One trainer (vpk_train_create) of sizes ``dims`` = (I, H6, H7, O) on a handle and stream of its own."""

    def __init__(self, dims, device=0, params=None, seed=0):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 4:
            raise ValueError("dims must be (I, H6, H7, O)")
        self.rt = Runtime(device)
        self.seed = int(seed)
        arr = (ctypes.c_int32 * 4)(*self.dims)
        self.rt.check(self.rt.lib.vpk_train_create(self.rt.h, arr))
        self.params = params if params is not None else SolverParams()
        self.set_params(self.params)

    def close(self):
        if getattr(self, "rt", None) is not None:
            self.rt.lib.vpk_train_destroy(self.rt.h)
            self.rt.handle.close()
            self.rt = None

    def shapes(self):
        i, h6, h7, o = self.dims
        return [(h6, i), (h6,), (h7, h6), (h7,), (o, h7), (o,)]

    def set_params(self, params):
        p = params.as_struct()
        self.rt.check(self.rt.lib.vpk_train_set_params(self.rt.h, ctypes.byref(p)))
        self.params = params

    def _in(self, fn, blobs):
        keep = []
        for a, shape in zip(blobs, self.shapes()):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError("expected a blob of shape %s, got %s" % (shape, a.shape))
            keep.append(a)
        arr = (ctypes.c_void_p * 6)(*[a.ctypes.data for a in keep])
        self.rt.check(fn(self.rt.h, arr))

    def _out(self, fn):
        out = [np.empty(shape, dtype=np.float32) for shape in self.shapes()]
        arr = (ctypes.c_void_p * 6)(*[a.ctypes.data for a in out])
        self.rt.check(fn(self.rt.h, arr))
        return out

    def load(self, blobs):
        """[W6, b6, W7, b7, W8, b8] float32 on the host; zeroes the momentum and the iteration."""
        self._in(self.rt.lib.vpk_train_load, blobs)

    def store(self):
        return self._out(self.rt.lib.vpk_train_store)

    def load_momentum(self, blobs):
        self._in(self.rt.lib.vpk_train_load_momentum, blobs)

    def store_momentum(self):
        return self._out(self.rt.lib.vpk_train_store_momentum)

    @property
    def iteration(self):
        it = ctypes.c_longlong()
        self.rt.check(self.rt.lib.vpk_train_get_iteration(self.rt.h, ctypes.byref(it)))
        return int(it.value)

    @iteration.setter
    def iteration(self, value):
        self.rt.check(self.rt.lib.vpk_train_set_iteration(self.rt.h, int(value)))

    def _dev(self, x, dtype, cols):
        """x (numpy or tensor) as a contiguous (B, cols) device tensor of ``dtype``, ordered on the trainer's stream"""
        rt = self.rt
        t = rt.torch
        if hasattr(x, "is_cuda"):
            if x.is_cuda:
                rt.stream.wait_stream(t.cuda.current_stream(x.device))
        else:
            x = t.from_numpy(np.ascontiguousarray(x))
        with rt.on_stream():
            x = x.to(device=rt.tdev, dtype=dtype)
            x = (x.reshape(x.shape[0], -1) if x.shape[0] else x.reshape(0, cols)).contiguous()
        if x.shape[1] != cols:
            raise ValueError("expected %d values per row, got %d" % (cols, x.shape[1]))
        return x

    def step(self, features, labels, masks=None):
        """One solver iteration on B <= 32 rows.  features (B, I), labels (B, O) in [0, 1]; masks: None (generated from the
        trainer's seed and the iteration) or (mask6 (B, H6), mask7 (B, H7)) of 0/1.  Returns (loss, sigout) device tensors;
        asynchronous: the step runs on the trainer's stream and the caller's current stream is made to wait for it."""
        rt = self.rt
        t = rt.torch
        i, h6, h7, o = self.dims
        x = self._dev(features, t.float32, i)
        lab = self._dev(labels, t.float32, o)
        b = int(x.shape[0])
        if lab.shape[0] != b:
            raise ValueError("features and labels differ in their batch")
        m6 = m7 = None
        if masks is not None and 1 <= b <= MAX_BATCH:
            m6, m7 = self._dev(masks[0], t.uint8, h6), self._dev(masks[1], t.uint8, h7)
            if m6.shape[0] != b or m7.shape[0] != b:
                raise ValueError("masks and features differ in their batch")
        with rt.on_stream():
            loss = t.empty((1,), dtype=t.float32, device=rt.tdev)
            sig = t.empty((b, o), dtype=t.float32, device=rt.tdev)
            rt.check(rt.lib.vpk_train_step(rt.h, rt.ptr(x), rt.ptr(lab), b, rt.ptr(m6), rt.ptr(m7), self.seed, rt.ptr(loss),
                                           rt.ptr(sig)))
            for buf in (x, lab, m6, m7):
                if buf is not None:
                    buf.record_stream(rt.stream)
        t.cuda.current_stream(rt.tdev).wait_stream(rt.stream)      # the results are safe to use on the caller's stream
        return loss[0], sig

    def evaluate(self, features, labels=None):
        """The TEST phase (no dropout) on any batch: (loss or None, sigout); changes no weight."""
        rt = self.rt
        t = rt.torch
        i, _, _, o = self.dims
        x = self._dev(features, t.float32, i)
        lab = self._dev(labels, t.float32, o) if labels is not None else None
        b = int(x.shape[0])
        if lab is not None and lab.shape[0] != b:
            raise ValueError("features and labels differ in their batch")
        with rt.on_stream():
            loss = t.empty((1,), dtype=t.float32, device=rt.tdev) if lab is not None else None
            sig = t.empty((b, o), dtype=t.float32, device=rt.tdev)
            rt.check(rt.lib.vpk_train_eval(rt.h, rt.ptr(x), rt.ptr(lab), b, rt.ptr(loss), rt.ptr(sig)))
            for buf in (x, lab):
                if buf is not None:
                    buf.record_stream(rt.stream)
        t.cuda.current_stream(rt.tdev).wait_stream(rt.stream)
        return (loss[0] if loss is not None else None), sig

    def synchronize(self):
        self.rt.synchronize()


class HeadTrainer(Head):
    """The head of ``net`` (a ``cnn.Net``) under the solver: features from the net's frozen conv stack, fp32 master weights
    of fc6-fc8 started from ``weights`` (the dict ``cnn.Net`` takes).  ``step`` and ``evaluate`` take uint8 / float rasters
    (B, 500, 500) or ready features (B, 57600)."""

    def __init__(self, net, weights, device=0, params=None, seed=0):
        Head.__init__(self, NET_DIMS, device=device, params=params, seed=seed)
        self.net = net
        self._weights = dict(weights)
        blobs = []
        for name in HEAD_LAYERS:
            blobs += [weights[name][0], weights[name][1]]
        self.load(blobs)

    def features(self, sphere):
        """pool5 of the rasters, flattened to (B, 57600) in Caffe's C x H x W order (a device tensor)."""
        if not hasattr(sphere, "is_cuda"):
            sphere = self.net.rt.torch.from_numpy(np.ascontiguousarray(sphere)).to(self.net.rt.tdev)
        _, tap = self.net.forward_device(sphere, tap=7)
        self.rt.stream.wait_stream(self.net.rt.stream)
        tap.record_stream(self.rt.stream)
        return tap.reshape(tap.shape[0], -1)

    def _features_of(self, x):
        return self.features(x) if len(x.shape) == 3 else x

    def step(self, sphere_or_features, labels, masks=None):
        labels = labels.reshape(labels.shape[0], -1)
        return Head.step(self, self._features_of(sphere_or_features), labels, masks)

    def evaluate(self, sphere_or_features, labels=None):
        if labels is not None:
            labels = labels.reshape(labels.shape[0], -1)
        loss, sig = Head.evaluate(self, self._features_of(sphere_or_features), labels)
        return loss, sig.reshape(-1, 20, 20)

    def weights(self):
        """The full weight dict: the conv layers as given, the head read back from the device."""
        out = dict(self._weights)
        blobs = self.store()
        for k, name in enumerate(HEAD_LAYERS):
            out[name] = (blobs[2 * k], blobs[2 * k + 1])
        return out

    def save_caffemodel(self, path):
        """Writes ``weights()`` as a caffemodel that evaluation.init_caffe reads (fc8 under the prototxt's name fc8_20x20)."""
        w = self.weights()
        layers = {}
        for name, _ in cnn.LAYER_SHAPES:
            layers["fc8_20x20" if name == "fc8" else name] = [w[name][0], w[name][1]]
        caffe_io.write_caffemodel(path, layers)
