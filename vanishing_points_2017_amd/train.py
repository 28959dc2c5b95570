"""Fine-tuning the net on the GPU: the reference's train/train_val.prototxt under train/solver.prototxt, without Caffe
(C-ABI: vpk_train_* in csrc/vpk_train.hip, vpk_convtrain_* in csrc/vpk_convtrain.hip).

``HeadTrainer`` keeps the conv stack frozen: ``HeadTrainer.features`` takes pool5 from the forward
(``Net.forward_device(sphere, tap=7)``) and a step trains the three InnerProduct layers on it -- 254.4 M of the net's 258 M
parameters; it is the cheaper flow when only the head is adapted.  ``NetTrainer`` trains all eight layers: a ``ConvStack`` at
the net's descriptor (conv1-5, LRN, the pools) below the head, on one handle and stream.  ``Head`` and ``ConvStack`` are the
C-ABI at any sizes.  There is no CPU fallback."""
import ctypes

import numpy as np

from . import _lib, caffe_io, cnn, coordinate_conversion
from .runtime import Runtime

HEAD_LAYERS = ("fc6", "fc7", "fc8")
CONV_LAYERS = ("conv1", "conv2", "conv3", "conv4", "conv5")
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

    def __init__(self, dims, device=0, params=None, seed=0, runtime=None):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 4:
            raise ValueError("dims must be (I, H6, H7, O)")
        self.rt = runtime if runtime is not None else Runtime(device)
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

    def step(self, features, labels, masks=None, want_dx=False):
        """One solver iteration on B <= 32 rows.  features (B, I), labels (B, O) in [0, 1]; masks: None (generated from the
        trainer's seed and the iteration) or (mask6 (B, H6), mask7 (B, H7)) of 0/1.  Returns (loss, sigout) device tensors
        and, with ``want_dx`` (vpk_train_step_dx), the (B, I) gradient with respect to the features as a third;
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
            dx = None
            if want_dx:
                dx = t.empty((b, i), dtype=t.float32, device=rt.tdev)
                rt.check(rt.lib.vpk_train_step_dx(rt.h, rt.ptr(x), rt.ptr(lab), b, rt.ptr(m6), rt.ptr(m7), self.seed,
                                                  rt.ptr(loss), rt.ptr(sig), rt.ptr(dx)))
            else:
                rt.check(rt.lib.vpk_train_step(rt.h, rt.ptr(x), rt.ptr(lab), b, rt.ptr(m6), rt.ptr(m7), self.seed, rt.ptr(loss),
                                               rt.ptr(sig)))
            for buf in (x, lab, m6, m7):
                if buf is not None:
                    buf.record_stream(rt.stream)
        t.cuda.current_stream(rt.tdev).wait_stream(rt.stream)      # the results are safe to use on the caller's stream
        return (loss[0], sig, dx) if want_dx else (loss[0], sig)

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


def conv_layer(out_channels, kernel, stride=1, pad=0, groups=1, relu=True):
    return _lib.StackLayer(kind=_lib.LAYER_CONV, out_channels=out_channels, kernel=kernel, stride=stride, pad=pad, groups=groups,
                           relu=int(bool(relu)))


def lrn_layer(local_size=5, alpha=1e-4, beta=0.75, k=1.0):
    return _lib.StackLayer(kind=_lib.LAYER_LRN, local_size=local_size, alpha=alpha, beta=beta, k=k)


def pool_layer(kernel=3, stride=2):
    return _lib.StackLayer(kind=_lib.LAYER_POOL, kernel=kernel, stride=stride)


def net_stack():
    """((C, H, W), layers) of the net's conv stack as the library exports it (vpk_convtrain_net_layers; needs no GPU)."""
    lib = _lib.load()
    n = lib.vpk_convtrain_net_layers(None, 0, None)
    layers = (_lib.StackLayer * n)()
    shape = (ctypes.c_int32 * 3)()
    lib.vpk_convtrain_net_layers(layers, n, shape)
    return tuple(shape), list(layers)


def _pool_out_size(size, kernel, stride):
    out = -((kernel - size) // stride) + 1              # Caffe's ceil mode
    return out - 1 if (out - 1) * stride >= size else out


def stack_shapes(in_shape, layers):
    """The output shape (C, H, W) of every layer under include/vpk.h's size rules (what the blobs of a step are read with)."""
    c, h, w = (int(v) for v in in_shape)
    out = []
    for d in layers:
        if d.kind == _lib.LAYER_CONV:
            c, h, w = d.out_channels, (h + 2 * d.pad - d.kernel) // d.stride + 1, (w + 2 * d.pad - d.kernel) // d.stride + 1
        elif d.kind == _lib.LAYER_POOL:
            h, w = (_pool_out_size(v, d.kernel, d.stride) for v in (h, w))
        out.append((c, h, w))
    return out


class ConvStack(object):
    """One conv trainer (vpk_convtrain_create) on ``in_shape`` = (C, H, W) and ``layers`` (conv_layer / lrn_layer /
    pool_layer descriptors), on a handle and stream of its own or on ``runtime``'s."""

    def __init__(self, in_shape, layers, device=0, params=None, runtime=None):
        self.in_shape = tuple(int(v) for v in in_shape)
        self.layers = list(layers)
        self.rt = runtime if runtime is not None else Runtime(device)
        self._own = runtime is None
        arr = (_lib.StackLayer * len(self.layers))(*self.layers)
        c, h, w = self.in_shape
        self.rt.check(self.rt.lib.vpk_convtrain_create(self.rt.h, c, h, w, arr, len(self.layers)))
        self.shapes = stack_shapes(self.in_shape, self.layers)
        self.batch = 0                       # of the last forward
        self.set_params(params if params is not None else SolverParams())

    def close(self):
        if getattr(self, "rt", None) is not None:
            self.rt.lib.vpk_convtrain_destroy(self.rt.h)
            if self._own:
                self.rt.handle.close()
            self.rt = None

    def blob_shapes(self):
        """[(OC, C / groups, K, K), (OC,)] per CONV layer, in stack order"""
        out, c = [], self.in_shape[0]
        for d, shape in zip(self.layers, self.shapes):
            if d.kind == _lib.LAYER_CONV:
                out += [(d.out_channels, c // d.groups, d.kernel, d.kernel), (d.out_channels,)]
            c = shape[0]
        return out

    def set_params(self, params):
        p = params.as_struct()
        self.rt.check(self.rt.lib.vpk_convtrain_set_params(self.rt.h, ctypes.byref(p)))
        self.params = params

    def _in(self, fn, blobs):
        shapes = self.blob_shapes()
        blobs = list(blobs)
        if len(blobs) != len(shapes):
            raise ValueError("expected %d blobs, got %d" % (len(shapes), len(blobs)))
        keep = []
        for a, shape in zip(blobs, shapes):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError("expected a blob of shape %s, got %s" % (shape, a.shape))
            keep.append(a)
        arr = (ctypes.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
        self.rt.check(fn(self.rt.h, arr))

    def _out(self, fn):
        out = [np.empty(shape, dtype=np.float32) for shape in self.blob_shapes()]
        arr = (ctypes.c_void_p * len(out))(*[a.ctypes.data for a in out])
        self.rt.check(fn(self.rt.h, arr))
        return out

    def load(self, blobs):
        """[W, b] of every CONV layer in stack order, float32 on the host; zeroes the momentum and the iteration."""
        self._in(self.rt.lib.vpk_convtrain_load, blobs)

    def store(self):
        return self._out(self.rt.lib.vpk_convtrain_store)

    def load_momentum(self, blobs):
        self._in(self.rt.lib.vpk_convtrain_load_momentum, blobs)

    def store_momentum(self):
        return self._out(self.rt.lib.vpk_convtrain_store_momentum)

    @property
    def iteration(self):
        it = ctypes.c_longlong()
        self.rt.check(self.rt.lib.vpk_convtrain_get_iteration(self.rt.h, ctypes.byref(it)))
        return int(it.value)

    @iteration.setter
    def iteration(self, value):
        self.rt.check(self.rt.lib.vpk_convtrain_set_iteration(self.rt.h, int(value)))

    def _dev(self, x, shape):
        """x (numpy or tensor) as a contiguous float32 device tensor (B,) + shape, ordered on the trainer's stream"""
        rt = self.rt
        t = rt.torch
        if hasattr(x, "is_cuda"):
            if x.is_cuda:
                rt.stream.wait_stream(t.cuda.current_stream(x.device))
        else:
            x = t.from_numpy(np.ascontiguousarray(x))
        with rt.on_stream():
            x = x.to(device=rt.tdev, dtype=t.float32).contiguous()
        if tuple(x.shape[1:]) != tuple(shape):
            x = x.reshape((x.shape[0],) + tuple(shape)) if x.shape[0] else x.reshape((0,) + tuple(shape))
        return x

    def forward(self, x):
        """The stack's forward on (B, C, H, W), 1 <= B <= 32; returns the last blob (B, C', H', W') as a device tensor.  Every
        layer's blobs stay in the library until the next forward (``read``)."""
        rt = self.rt
        t = rt.torch
        x = self._dev(x, self.in_shape)
        b = int(x.shape[0])
        with rt.on_stream():
            top = t.empty((b,) + self.shapes[-1], dtype=t.float32, device=rt.tdev)
            rt.check(rt.lib.vpk_convtrain_forward(rt.h, rt.ptr(x), b, rt.ptr(top)))
            x.record_stream(rt.stream)
        self.batch = b
        t.cuda.current_stream(rt.tdev).wait_stream(rt.stream)
        return top

    def backward(self, d_top, want_dx=False):
        """Back-propagation of d_top (the gradient with respect to ``forward``'s result) and the solver's update of every CONV
        layer.  Returns the gradient with respect to the input with ``want_dx``, else None (and then it is not computed)."""
        rt = self.rt
        t = rt.torch
        d = self._dev(d_top, self.shapes[-1])
        if self.batch and d.shape[0] != self.batch:
            raise ValueError("d_top has %d images, the forward had %d" % (d.shape[0], self.batch))
        with rt.on_stream():
            dx = t.empty((self.batch,) + self.in_shape, dtype=t.float32, device=rt.tdev) if want_dx else None
            rt.check(rt.lib.vpk_convtrain_backward(rt.h, rt.ptr(d), rt.ptr(dx)))
            d.record_stream(rt.stream)
        t.cuda.current_stream(rt.tdev).wait_stream(rt.stream)
        return dx

    def read(self, layer, kind="output"):
        """One kept blob of ``layer`` as a device tensor: "output" (float32), "index" (int32, POOL layers: the flat index of
        the maximum inside the input plane), "gradient" (float32, with respect to the layer's output, after a backward) or
        "scale" (float32, LRN layers: s)."""
        rt = self.rt
        t = rt.torch
        code = {"output": _lib.BLOB_OUTPUT, "index": _lib.BLOB_POOL_INDEX, "gradient": _lib.BLOB_GRADIENT,
                "scale": _lib.BLOB_LRN_SCALE}[kind]
        with rt.on_stream():
            out = t.empty((self.batch,) + self.shapes[layer], dtype=t.int32 if kind == "index" else t.float32, device=rt.tdev)
            rt.check(rt.lib.vpk_convtrain_read(rt.h, int(layer), code, rt.ptr(out)))
        t.cuda.current_stream(rt.tdev).wait_stream(rt.stream)
        return out

    def synchronize(self):
        self.rt.synchronize()


class NetTrainer(object):
    """All eight layers of the net under the solver: a ``ConvStack`` at the net's descriptor and the head above it on one
    handle and stream, fp32 master weights started from ``weights`` (the dict ``cnn.Net`` takes), inputs as Caffe's data
    layer makes them: the raster minus ``mean`` (transform_param.mean_file)."""

    def __init__(self, weights, mean, device=0, params=None, seed=0):
        params = params if params is not None else SolverParams()
        self.head = Head(NET_DIMS, device=device, params=params, seed=seed)
        self.rt = self.head.rt
        shape, layers = net_stack()
        self.stack = ConvStack(shape, layers, params=params, runtime=self.rt)
        self.params = params
        blobs = []
        for name in CONV_LAYERS:
            blobs += [weights[name][0], weights[name][1]]
        self.stack.load(blobs)
        blobs = []
        for name in HEAD_LAYERS:
            blobs += [weights[name][0], weights[name][1]]
        self.head.load(blobs)
        t = self.rt.torch
        with self.rt.on_stream():
            self.mean = t.from_numpy(np.ascontiguousarray(np.asarray(mean, dtype=np.float32).reshape(500, 500))).to(self.rt.tdev)

    def close(self):
        if getattr(self, "rt", None) is not None:
            self.stack.close()
            self.head.close()
            self.rt = None

    def set_params(self, params):
        self.stack.set_params(params)
        self.head.set_params(params)
        self.params = params

    @property
    def iteration(self):
        it = self.head.iteration
        if self.stack.iteration != it:
            raise _lib.VpkError("the head is at iteration %d, the conv stack at %d" % (it, self.stack.iteration))
        return it

    @iteration.setter
    def iteration(self, value):
        self.head.iteration = value
        self.stack.iteration = value

    def _data(self, rasters):
        """(B, 500, 500) uint8 / float rasters -> the data blob (B, 1, 500, 500): float32 raster minus the mean"""
        x = self.stack._dev(rasters, (500, 500))
        with self.rt.on_stream():
            return (x - self.mean).reshape(x.shape[0], 1, 500, 500)

    def step(self, rasters, labels, masks=None):
        """One solver iteration of the whole net on B <= 32 rasters: the stack's forward, the head's step with the gradient
        with respect to pool5 written out, the stack's backward and update.  Returns (loss, sigout) like ``Head.step``."""
        if not 1 <= int(rasters.shape[0]) <= MAX_BATCH:
            raise _lib.VpkError("libvpk error -5: a step takes 1..%d rasters, got %d" % (MAX_BATCH, rasters.shape[0]))
        labels = labels.reshape(labels.shape[0], -1)
        top = self.stack.forward(self._data(rasters))
        loss, sig, dx = self.head.step(top.reshape(top.shape[0], -1), labels, masks, want_dx=True)
        self.stack.backward(dx)
        return loss, sig

    def features(self, rasters):
        """pool5 of the rasters under the trainer's own conv weights, (B, 57600); any B, in chunks of 32"""
        t = self.rt.torch
        x = self._data(rasters)
        tops = [self.stack.forward(x[i:i + MAX_BATCH]) for i in range(0, int(x.shape[0]), MAX_BATCH)]
        return t.cat(tops).reshape(int(x.shape[0]), -1)

    def evaluate(self, rasters, labels=None):
        """The TEST phase of the whole net: (loss or None, response maps (B, 20, 20)); changes no weight."""
        if labels is not None:
            labels = labels.reshape(labels.shape[0], -1)
        loss, sig = self.head.evaluate(self.features(rasters), labels)
        return loss, sig.reshape(-1, 20, 20)

    def weights(self):
        """All eight layers read back from the device, as the dict ``cnn.Net`` takes."""
        out = {}
        blobs = self.stack.store()
        for k, name in enumerate(CONV_LAYERS):
            out[name] = (blobs[2 * k], blobs[2 * k + 1])
        blobs = self.head.store()
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

    def synchronize(self):
        self.rt.synchronize()
