"""Fine-tuning the net on the GPU: the reference's train/train_val.prototxt under train/solver.prototxt, without Caffe
(C-ABI: vpk_train_* in csrc/vpk_train.hip, vpk_convtrain_* in csrc/vpk_convtrain.hip).

``HeadTrainer`` keeps the conv stack frozen: ``HeadTrainer.features`` takes pool5 from the forward
(``Net.forward_device(sphere, tap=7)``) and a step trains the three InnerProduct layers on it -- 254.4 M of the net's 258 M
parameters; it is the cheaper flow when only the head is adapted.  ``NetTrainer`` trains all eight layers: a ``ConvStack`` at
the net's descriptor (conv1-5, LRN, the pools) below the head, on one handle and stream.  ``Head`` and ``ConvStack`` are the
C-ABI at any sizes, ``StackTrainer`` the two on one handle at any geometry (``NetTrainer`` is it at the net's).

``TrainSet`` keeps the lines and ground-truth VPs of a data set on the device and makes the batch of an iteration there
(vpk_trainset_* in csrc/vpk_trainset.hip, then vpk_sphere_raster): what train_val.prototxt:1-62 reads from LMDB, with
``Augment``'s affine maps of the image plane.  ``Solver`` is solver.prototxt's loop around a trainer and a set: iterations,
test passes, displays, snapshots and resuming.  There is no CPU fallback."""
import contextlib
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


def _to_device(rt, x, dtype, shape):
    """x (numpy or tensor) as a contiguous device tensor (B,) + shape of ``dtype``, ordered on the trainer's stream"""
    t = rt.torch
    shape = tuple(int(v) for v in shape)
    if hasattr(x, "is_cuda"):
        if x.is_cuda:
            rt.stream.wait_stream(t.cuda.current_stream(x.device))
    else:
        x = t.from_numpy(np.ascontiguousarray(x))
    with rt.on_stream():
        x = x.to(device=rt.tdev, dtype=dtype).contiguous()
    b, row = int(x.shape[0]), int(np.prod(shape))
    if tuple(x.shape[1:]) != shape:
        if x.numel() != b * row:
            raise ValueError("expected %d values per row, got %d" % (row, x.numel() // max(b, 1)))
        x = x.reshape((b,) + shape)
    return x


@contextlib.contextmanager
def _on_stream(rt, *inputs):
    """The body runs on the trainer's stream: what it allocates belongs to that stream and ``inputs`` (device tensors or
    None) are kept alive for it; afterwards the caller's current stream waits for it, so the results are safe to use there.
    Nothing of this happens after a body that raises."""
    with rt.on_stream():
        yield
        for buf in inputs:
            if buf is not None:
                buf.record_stream(rt.stream)
    rt.torch.cuda.current_stream(rt.tdev).wait_stream(rt.stream)


def _blob_list(weights, names):
    """[W, b, W, b, ...] of the layers ``names`` from a weight dict"""
    return [a for name in names for a in weights[name][:2]]


def _blob_dict(names, blobs):
    return {name: (blobs[2 * k], blobs[2 * k + 1]) for k, name in enumerate(names)}


def _response_maps(sigout):
    return sigout.reshape(-1, 20, 20)


def _save_caffemodel(self, path):
    """Writes ``weights()`` as a caffemodel that evaluation.init_caffe reads (fc8 under the prototxt's name fc8_20x20)."""
    w = self.weights()
    layers = {}
    for name, _ in cnn.LAYER_SHAPES:
        layers["fc8_20x20" if name == "fc8" else name] = [w[name][0], w[name][1]]
    caffe_io.write_caffemodel(path, layers)


class _Params(object):
    """What ``Head`` and ``ConvStack`` share: the master weights and momentum as host blobs of ``blob_shapes()``, the solver's
    numbers and the iteration, through the C-ABI functions PREFIX + name.  ``_own``: close() closes the handle too."""

    PREFIX = None

    def _call(self, name, *args):
        self.rt.check(getattr(self.rt.lib, self.PREFIX + name)(self.rt.h, *args))

    def close(self):
        if getattr(self, "rt", None) is not None:
            getattr(self.rt.lib, self.PREFIX + "destroy")(self.rt.h)
            if self._own:
                self.rt.handle.close()
            self.rt = None

    def set_params(self, params):
        self._call("set_params", ctypes.byref(params.as_struct()))
        self.params = params

    def _in(self, name, blobs):
        shapes, blobs = self.blob_shapes(), list(blobs)
        if len(blobs) != len(shapes):
            raise ValueError("expected %d blobs, got %d" % (len(shapes), len(blobs)))
        keep = [np.ascontiguousarray(a, dtype=np.float32) for a in blobs]
        for a, shape in zip(keep, shapes):
            if a.shape != shape:
                raise ValueError("expected a blob of shape %s, got %s" % (shape, a.shape))
        self._call(name, (ctypes.c_void_p * len(keep))(*[a.ctypes.data for a in keep]))

    def _out(self, name):
        out = [np.empty(shape, dtype=np.float32) for shape in self.blob_shapes()]
        self._call(name, (ctypes.c_void_p * len(out))(*[a.ctypes.data for a in out]))
        return out

    def load(self, blobs):
        """[W, b] of every layer in order (``blob_shapes()``), float32 on the host; zeroes the momentum and the iteration."""
        self._in("load", blobs)

    def store(self):
        return self._out("store")

    def load_momentum(self, blobs):
        self._in("load_momentum", blobs)

    def store_momentum(self):
        return self._out("store_momentum")

    @property
    def iteration(self):
        it = ctypes.c_longlong()
        self._call("get_iteration", ctypes.byref(it))
        return int(it.value)

    @iteration.setter
    def iteration(self, value):
        self._call("set_iteration", int(value))

    def synchronize(self):
        self.rt.synchronize()


class Head(_Params):
    """One trainer (vpk_train_create) of sizes ``dims`` = (I, H6, H7, O) on a handle and stream of its own."""

    PREFIX = "vpk_train_"
    _own = True

    def __init__(self, dims, device=0, params=None, seed=0, runtime=None):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 4:
            raise ValueError("dims must be (I, H6, H7, O)")
        self.rt = runtime if runtime is not None else Runtime(device)
        self.seed = int(seed)
        self._call("create", (ctypes.c_int32 * 4)(*self.dims))
        self.params = params if params is not None else SolverParams()
        self.set_params(self.params)

    def shapes(self):
        i, h6, h7, o = self.dims
        return [(h6, i), (h6,), (h7, h6), (h7,), (o, h7), (o,)]

    blob_shapes = shapes                 # [W6, b6, W7, b7, W8, b8]

    def step(self, features, labels, masks=None, want_dx=False):
        """One solver iteration on B <= 32 rows.  features (B, I), labels (B, O) in [0, 1]; masks: None (generated from the
        trainer's seed and the iteration) or (mask6 (B, H6), mask7 (B, H7)) of 0/1.  Returns (loss, sigout) device tensors
        and, with ``want_dx`` (vpk_train_step_dx), the (B, I) gradient with respect to the features as a third;
        asynchronous: the step runs on the trainer's stream and the caller's current stream is made to wait for it."""
        rt = self.rt
        t = rt.torch
        i, h6, h7, o = self.dims
        x = _to_device(rt, features, t.float32, (i,))
        lab = _to_device(rt, labels, t.float32, (o,))
        b = int(x.shape[0])
        if lab.shape[0] != b:
            raise ValueError("features and labels differ in their batch")
        m6 = m7 = None
        if masks is not None and 1 <= b <= MAX_BATCH:
            m6, m7 = _to_device(rt, masks[0], t.uint8, (h6,)), _to_device(rt, masks[1], t.uint8, (h7,))
            if m6.shape[0] != b or m7.shape[0] != b:
                raise ValueError("masks and features differ in their batch")
        with _on_stream(rt, x, lab, m6, m7):
            loss = t.empty((1,), dtype=t.float32, device=rt.tdev)
            sig = t.empty((b, o), dtype=t.float32, device=rt.tdev)
            args = (rt.ptr(x), rt.ptr(lab), b, rt.ptr(m6), rt.ptr(m7), self.seed, rt.ptr(loss), rt.ptr(sig))
            dx = None
            if want_dx:
                dx = t.empty((b, i), dtype=t.float32, device=rt.tdev)
                self._call("step_dx", *(args + (rt.ptr(dx),)))
            else:
                self._call("step", *args)
        return (loss[0], sig, dx) if want_dx else (loss[0], sig)

    def evaluate(self, features, labels=None):
        """The TEST phase (no dropout) on any batch: (loss or None, sigout); changes no weight."""
        rt = self.rt
        t = rt.torch
        i, _, _, o = self.dims
        x = _to_device(rt, features, t.float32, (i,))
        lab = _to_device(rt, labels, t.float32, (o,)) if labels is not None else None
        b = int(x.shape[0])
        if lab is not None and lab.shape[0] != b:
            raise ValueError("features and labels differ in their batch")
        with _on_stream(rt, x, lab):
            loss = t.empty((1,), dtype=t.float32, device=rt.tdev) if lab is not None else None
            sig = t.empty((b, o), dtype=t.float32, device=rt.tdev)
            self._call("eval", rt.ptr(x), rt.ptr(lab), b, rt.ptr(loss), rt.ptr(sig))
        return (loss[0] if loss is not None else None), sig


class HeadTrainer(Head):
    """The head of ``net`` (a ``cnn.Net``) under the solver: features from the net's frozen conv stack, fp32 master weights
    of fc6-fc8 started from ``weights`` (the dict ``cnn.Net`` takes).  ``step`` and ``evaluate`` take uint8 / float rasters
    (B, 500, 500) or ready features (B, 57600)."""

    def __init__(self, net, weights, device=0, params=None, seed=0):
        Head.__init__(self, NET_DIMS, device=device, params=params, seed=seed)
        self.net = net
        self._weights = dict(weights)
        self.load(_blob_list(weights, HEAD_LAYERS))

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
        return loss, _response_maps(sig)

    def weights(self):
        """The full weight dict: the conv layers as given, the head read back from the device."""
        return dict(self._weights, **_blob_dict(HEAD_LAYERS, self.store()))

    save_caffemodel = _save_caffemodel


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


class ConvStack(_Params):
    """One conv trainer (vpk_convtrain_create) on ``in_shape`` = (C, H, W) and ``layers`` (conv_layer / lrn_layer /
    pool_layer descriptors), on a handle and stream of its own or on ``runtime``'s."""

    PREFIX = "vpk_convtrain_"

    def __init__(self, in_shape, layers, device=0, params=None, runtime=None):
        self.in_shape = tuple(int(v) for v in in_shape)
        self.layers = list(layers)
        self.rt = runtime if runtime is not None else Runtime(device)
        self._own = runtime is None
        arr = (_lib.StackLayer * len(self.layers))(*self.layers)
        c, h, w = self.in_shape
        self._call("create", c, h, w, arr, len(self.layers))
        self.shapes = stack_shapes(self.in_shape, self.layers)
        self.batch = 0                       # of the last forward
        self.set_params(params if params is not None else SolverParams())

    def blob_shapes(self):
        """[(OC, C / groups, K, K), (OC,)] per CONV layer, in stack order"""
        out, c = [], self.in_shape[0]
        for d, shape in zip(self.layers, self.shapes):
            if d.kind == _lib.LAYER_CONV:
                out += [(d.out_channels, c // d.groups, d.kernel, d.kernel), (d.out_channels,)]
            c = shape[0]
        return out

    def forward(self, x):
        """The stack's forward on (B, C, H, W), 1 <= B <= 32; returns the last blob (B, C', H', W') as a device tensor.  Every
        layer's blobs stay in the library until the next forward (``read``)."""
        rt = self.rt
        t = rt.torch
        x = _to_device(rt, x, t.float32, self.in_shape)
        b = int(x.shape[0])
        with _on_stream(rt, x):
            top = t.empty((b,) + self.shapes[-1], dtype=t.float32, device=rt.tdev)
            self._call("forward", rt.ptr(x), b, rt.ptr(top))
            self.batch = b
        return top

    def backward(self, d_top, want_dx=False):
        """Back-propagation of d_top (the gradient with respect to ``forward``'s result) and the solver's update of every CONV
        layer.  Returns the gradient with respect to the input with ``want_dx``, else None (and then it is not computed)."""
        rt = self.rt
        t = rt.torch
        d = _to_device(rt, d_top, t.float32, self.shapes[-1])
        if self.batch and d.shape[0] != self.batch:
            raise ValueError("d_top has %d images, the forward had %d" % (d.shape[0], self.batch))
        with _on_stream(rt, d):
            dx = t.empty((self.batch,) + self.in_shape, dtype=t.float32, device=rt.tdev) if want_dx else None
            self._call("backward", rt.ptr(d), rt.ptr(dx))
        return dx

    def read(self, layer, kind="output"):
        """One kept blob of ``layer`` as a device tensor: "output" (float32), "index" (int32, POOL layers: the flat index of
        the maximum inside the input plane), "gradient" (float32, with respect to the layer's output, after a backward) or
        "scale" (float32, LRN layers: s)."""
        rt = self.rt
        t = rt.torch
        code = {"output": _lib.BLOB_OUTPUT, "index": _lib.BLOB_POOL_INDEX, "gradient": _lib.BLOB_GRADIENT,
                "scale": _lib.BLOB_LRN_SCALE}[kind]
        with _on_stream(rt):
            out = t.empty((self.batch,) + self.shapes[layer], dtype=t.int32 if kind == "index" else t.float32, device=rt.tdev)
            self._call("read", int(layer), code, rt.ptr(out))
        return out


class StackTrainer(object):
    """A whole net under the solver at any geometry: a ``ConvStack`` on ``in_shape`` = (C, H, W) and ``layers`` below a ``Head``
    of sizes ``dims`` = (I, H6, H7, O) on one handle and stream, I the stack's flattened output.  ``weights``: (the stack's
    blobs as ``ConvStack.load`` takes them, the head's six as ``Head.load`` does).  Inputs are (B,) + in_shape or anything
    that reshapes to it (uint8 / float), less ``mean`` (broadcast to in_shape) when one is given."""

    INPUTS = "inputs"                    # what a step's refusal calls them

    def __init__(self, in_shape, layers, dims, weights, mean=None, device=0, params=None, seed=0):
        params = params if params is not None else SolverParams()
        self.in_shape = tuple(int(v) for v in in_shape)
        self.head = Head(dims, device=device, params=params, seed=seed)
        self.rt = self.head.rt
        try:
            self.stack = ConvStack(self.in_shape, layers, params=params, runtime=self.rt)
            flat = int(np.prod(self.stack.shapes[-1]))
            if flat != self.head.dims[0]:
                raise ValueError("the stack ends in %d values per image, the head takes %d" % (flat, self.head.dims[0]))
            self.params = params
            self.stack.load(weights[0])
            self.head.load(weights[1])
        except Exception:
            self.close()
            raise
        self.mean = None
        if mean is not None:
            t = self.rt.torch
            m = np.array(np.broadcast_to(np.asarray(mean, dtype=np.float32), self.in_shape))       # a writable copy
            with self.rt.on_stream():
                self.mean = t.from_numpy(m).to(self.rt.tdev)

    def close(self):
        if getattr(self, "rt", None) is not None:
            if getattr(self, "stack", None) is not None:
                self.stack.close()
            self.head.close()
            self.rt = None

    def set_params(self, params):
        self.head.set_params(params)         # the stricter rule first: a refusal leaves both halves as they were
        self.stack.set_params(params)
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

    def _data(self, x):
        x = _to_device(self.rt, x, self.rt.torch.float32, self.in_shape)
        if self.mean is None:
            return x
        with self.rt.on_stream():
            return x - self.mean

    def step(self, x, labels, masks=None):
        """One solver iteration of the whole stack on B <= 32 inputs; returns (loss, sigout (B, O)) like ``Head.step``."""
        if not 1 <= int(x.shape[0]) <= MAX_BATCH:
            raise _lib.VpkError("libvpk error -5: a step takes 1..%d %s, got %d" % (MAX_BATCH, self.INPUTS, x.shape[0]))
        labels = labels.reshape(labels.shape[0], -1)
        top = self.stack.forward(self._data(x))
        loss, sig, dx = self.head.step(top.reshape(top.shape[0], -1), labels, masks, want_dx=True)
        self.stack.backward(dx)
        return loss, sig

    def features(self, x):
        """The stack's flattened output (B, I) under the trainer's own weights; any B, in chunks of 32"""
        t = self.rt.torch
        x = self._data(x)
        tops = [self.stack.forward(x[i:i + MAX_BATCH]) for i in range(0, int(x.shape[0]), MAX_BATCH)]
        return t.cat(tops).reshape(int(x.shape[0]), -1)

    def evaluate(self, x, labels=None):
        """The TEST phase of the whole stack: (loss or None, sigout (B, O)); changes no weight."""
        if labels is not None:
            labels = labels.reshape(labels.shape[0], -1)
        return self.head.evaluate(self.features(x), labels)

    def synchronize(self):
        self.rt.synchronize()

    def state(self):
        """Weights, momentum and iteration of both halves (host arrays), and the seed that keys the dropout masks."""
        return {"iteration": self.iteration, "seed": self.head.seed,
                "conv_weights": self.stack.store(), "conv_momentum": self.stack.store_momentum(),
                "head_weights": self.head.store(), "head_momentum": self.head.store_momentum()}

    def load_state(self, d):
        self.stack.load(d["conv_weights"])
        self.stack.load_momentum(d["conv_momentum"])
        self.head.load(d["head_weights"])
        self.head.load_momentum(d["head_momentum"])
        self.head.seed = int(d["seed"])
        self.iteration = int(d["iteration"])


class NetTrainer(StackTrainer):
    """All eight layers of the net under the solver: a ``ConvStack`` at the net's descriptor and the head above it on one
    handle and stream, fp32 master weights started from ``weights`` (the dict ``cnn.Net`` takes), inputs as Caffe's data
    layer makes them: the raster minus ``mean`` (transform_param.mean_file).  ``StackTrainer`` at the net's geometry, with
    the response maps as (B, 20, 20) and the weights as ``cnn.Net``'s dict."""

    INPUTS = "rasters"

    def __init__(self, weights, mean, device=0, params=None, seed=0):
        shape, layers = net_stack()
        blobs = (_blob_list(weights, CONV_LAYERS), _blob_list(weights, HEAD_LAYERS))
        StackTrainer.__init__(self, shape, layers, NET_DIMS, blobs, mean=np.asarray(mean, dtype=np.float32).reshape(500, 500),
                              device=device, params=params, seed=seed)

    def evaluate(self, rasters, labels=None):
        """The TEST phase of the whole net: (loss or None, response maps (B, 20, 20)); changes no weight."""
        loss, sig = StackTrainer.evaluate(self, rasters, labels)
        return loss, _response_maps(sig)

    def weights(self):
        """All eight layers read back from the device, as the dict ``cnn.Net`` takes."""
        return dict(_blob_dict(CONV_LAYERS, self.stack.store()), **_blob_dict(HEAD_LAYERS, self.head.store()))

    save_caffemodel = _save_caffemodel


# ---- the training set on the device, its augmentation and the solver's loop (C-ABI: vpk_trainset_* in csrc/vpk_trainset.hip) ----
_M64 = (1 << 64) - 1
DRAW_LAYER, ORDER_LAYER = 0x41, 0x53          # csrc/trainset_device.hpp
MAX_MEAN_IMAGES = (2 ** 32 - 1) // 255


def mix64(z):
    """csrc/train_device.hpp's mix64 (the finaliser of splitmix64) on a Python integer"""
    z &= _M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z


def mask_key(seed, iteration, layer, b):
    """csrc/train_device.hpp's mask_key on Python integers"""
    h0 = mix64((seed + 0x9E3779B97F4A7C15 * (iteration + 1)) & _M64)
    return mix64(h0 ^ ((layer << 32) | b))


def draws(seed, iteration, b, count):
    """u_0 .. u_{count-1} of batch slot ``b`` at ``iteration`` (csrc/trainset_device.hpp): float64 in [0, 1), a pure function
    of (seed, iteration, b, k)."""
    key = mask_key(int(seed), int(iteration), DRAW_LAYER, int(b))
    return np.array([(mix64(key ^ k) >> 11) * 2.0 ** -53 for k in range(count)], dtype=np.float64)


class Augment(object):
    """One affine map of the image plane per example, H = T(tx, ty) . S(s) . R(theta) . diag(m, 1, 1), applied to the
    example's lines and ground-truth VPs alike (vpk_trainset_batch), so the labels of an augmented example are exact.

    The reference ships no augmentation: its TRAIN data layer has a mean file and nothing else
    (train_val.prototxt:1-62), which is this class's default, the identity.  The four knobs are this project's own:
    max_rotation (radians, theta uniform in +-max_rotation), max_scale (>= 1, log s uniform in +-log max_scale), max_shift
    (normalised image units, tx and ty uniform in +-max_shift) and mirror (the probability of x -> -x)."""

    def __init__(self, max_rotation=0.0, max_scale=1.0, max_shift=0.0, mirror=0.0):
        self.max_rotation = float(max_rotation)
        self.max_scale = float(max_scale)
        self.max_shift = float(max_shift)
        self.mirror = float(mirror)
        if not (self.max_scale >= 1.0 and np.isfinite(self.max_scale)):
            raise ValueError("max_scale must be a finite number >= 1")
        if not (0.0 <= self.mirror <= 1.0):
            raise ValueError("mirror is a probability")

    def is_identity(self):
        return self.max_rotation == 0.0 and self.max_scale == 1.0 and self.max_shift == 0.0 and self.mirror == 0.0

    def as_dict(self):
        return {"max_rotation": self.max_rotation, "max_scale": self.max_scale, "max_shift": self.max_shift,
                "mirror": self.mirror}

    def transforms(self, seed, iteration, batch):
        """(batch, 6) float64 rows h00 h01 h02 h10 h11 h12 from the draws u_0 .. u_4 of every slot"""
        out = np.zeros((int(batch), 6), dtype=np.float64)
        for b in range(int(batch)):
            u = draws(seed, iteration, b, 5)
            theta = (2.0 * u[0] - 1.0) * self.max_rotation
            m = -1.0 if u[1] < self.mirror else 1.0
            s = np.exp((2.0 * u[2] - 1.0) * np.log(self.max_scale))
            tx = (2.0 * u[3] - 1.0) * self.max_shift
            ty = (2.0 * u[4] - 1.0) * self.max_shift
            c, sn = np.cos(theta), np.sin(theta)
            out[b] = (s * c * m, -(s * sn), tx, s * sn * m, s * c, ty)
        return out


def _host_prefix(counts):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    return off


class TrainSet(object):
    """The lines and ground-truth VPs of a whole data set on the device: what train_val.prototxt:1-62 reads from LMDB.
    ``batch`` gathers the examples of an iteration, maps each by its transform, rasterises the lines and writes the label
    maps; no pixel and no label crosses to or from the host.

    lines: a list of (N_i, 3) homogeneous lines; vps: a list of (V_i, 3) vanishing points in the normalised frame (any
    length, either sign; an empty array for none).  size, alpha: the raster's; grid: the label map's shape."""

    def __init__(self, lines, vps, size=500, grid=(20, 20), alpha=0.1, device=0, runtime=None):
        from .runtime import get_runtime
        rt = runtime if runtime is not None else get_runtime(device)
        lines = [np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in lines]
        cat = np.ascontiguousarray(np.concatenate(lines, 0)) if lines else np.zeros((0, 3))
        with rt.on_stream():
            l_dev = rt.torch.from_numpy(cat).to(rt.tdev)
        self._setup(rt, l_dev, _host_prefix([a.shape[0] for a in lines]), vps, size, grid, alpha)

    def _setup(self, rt, l_dev, line_offsets, vps, size, grid, alpha):
        self.rt = rt
        self.size, self.alpha = int(size), float(alpha)
        self.grid = (int(grid[0]), int(grid[1]))
        self.line_offsets = np.ascontiguousarray(line_offsets, dtype=np.int64)
        self.n = int(self.line_offsets.shape[0] - 1)
        vps = [np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in vps]
        if self.n < 1 or len(vps) != self.n:
            raise ValueError("a training set needs at least one image and one VP array per image (%d images, %d VP arrays)"
                             % (self.n, len(vps)))
        if int(l_dev.shape[0]) != int(self.line_offsets[-1]):
            raise ValueError("the line offsets end at %d, the store has %d lines" % (self.line_offsets[-1], l_dev.shape[0]))
        if self.line_offsets[0] != 0 or (np.diff(self.line_offsets) < 0).any():
            raise ValueError("the line offsets must rise from 0")
        self.vp_offsets = _host_prefix([a.shape[0] for a in vps])
        self.l = l_dev
        with rt.on_stream():
            self.vps = rt.torch.from_numpy(np.ascontiguousarray(np.concatenate(vps, 0))).to(rt.tdev)
        rt.synchronize()
        self._orders = {}

    @classmethod
    def from_frontend(cls, front, vps, size=500, grid=(20, 20), alpha=0.1, device=0, runtime=None):
        """From ``frontend.lines_batch_device``'s dict: its device ``l`` is kept as the store, without a host copy."""
        from .runtime import get_runtime
        self = cls.__new__(cls)
        rt = runtime if runtime is not None else get_runtime(device)
        l_dev = front["l"]
        if l_dev.dtype != rt.torch.float64 or not l_dev.is_contiguous():
            raise ValueError("front['l'] must be a contiguous float64 device tensor")
        self._setup(rt, l_dev, front["offsets"], vps, size, grid, alpha)
        return self

    @classmethod
    def from_scenes(cls, scenes, **kw):
        """From ``synth`` scenes (or any dicts with 'l' and 'true_vps', e.g. a data set after
        ``ground_truth.load_ground_truth``)."""
        return cls([s["l"] for s in scenes], [s["true_vps"] for s in scenes], **kw)

    def __len__(self):
        return self.n

    def order(self, seed, epoch, shuffle):
        """The order in which epoch ``epoch`` visits the examples: 0 .. n-1 without ``shuffle`` (Caffe's cursor), else the
        stable argsort of mix64(mask_key(seed, epoch, 0x53, 0) ^ i)."""
        if not shuffle:
            return np.arange(self.n, dtype=np.int64)
        key = (int(seed), int(epoch))
        if key not in self._orders:
            if len(self._orders) >= 4:
                self._orders.clear()
            k0 = mask_key(int(seed), int(epoch), ORDER_LAYER, 0)
            keys = np.array([mix64(k0 ^ i) for i in range(self.n)], dtype=np.uint64)
            self._orders[key] = np.argsort(keys, kind="stable").astype(np.int64)
        return self._orders[key]

    def indices(self, iteration, batch, seed=0, shuffle=False):
        """The examples of an iteration (host int32): position iteration * batch + b of the endless sequence of epochs; a
        batch that crosses an epoch's end continues in the next epoch's order."""
        pos = int(iteration) * int(batch) + np.arange(int(batch), dtype=np.int64)
        if not shuffle:
            return (pos % self.n).astype(np.int32)
        return np.array([self.order(seed, p // self.n, True)[p % self.n] for p in pos.tolist()], dtype=np.int32)

    def batch_parts(self, iteration, batch, seed=0, augment=None, shuffle=False, check=False, indices=None, transforms=None):
        """``batch`` with everything it made: a dict of rasters, labels, l_out (sum x 3), vp_out (sum V x 3), cell_out (int32
        per VP) as device tensors and index, offsets (lines), vp_offsets, transforms (None: the identity) on the host.
        ``indices`` / ``transforms`` replace the iteration's own.  One vpk_trainset_batch and one vpk_sphere_raster call;
        nothing is read back unless ``check`` asks for the raster's truncation flags (that waits)."""
        from .sphere_mapping import raster_batch_device, raster_flags
        rt = self.rt
        t = rt.torch
        index = np.ascontiguousarray(self.indices(iteration, batch, seed, shuffle) if indices is None else indices, dtype=np.int32)
        b = int(index.shape[0])
        if transforms is None and augment is not None and not augment.is_identity():
            transforms = augment.transforms(seed, iteration, b)
        if transforms is not None:
            transforms = np.ascontiguousarray(transforms, dtype=np.float64).reshape(b, 6)
        ok = (index >= 0) & (index < self.n)
        safe = np.where(ok, index, 0)
        offsets = _host_prefix(self.line_offsets[safe + 1] - self.line_offsets[safe])
        vp_offsets = _host_prefix(self.vp_offsets[safe + 1] - self.vp_offsets[safe])
        cells = self.grid[0] * self.grid[1]
        cur = t.cuda.current_stream(rt.tdev)
        with t.cuda.device(rt.tdev):          # the outputs belong to the caller's stream, where its consumers are ordered
            l_out = t.empty((int(offsets[-1]), 3), dtype=t.float64, device=rt.tdev)
            vp_out = t.empty((int(vp_offsets[-1]), 3), dtype=t.float64, device=rt.tdev)
            cell_out = t.empty((int(vp_offsets[-1]),), dtype=t.int32, device=rt.tdev)
            labels = t.empty((b, cells), dtype=t.float32, device=rt.tdev)
            rasters = t.empty((b, self.size, self.size), dtype=t.uint8, device=rt.tdev)
        rt.stream.wait_stream(cur)
        vp = ctypes.c_void_p
        with _on_stream(rt):
            rt.check(rt.lib.vpk_trainset_batch(
                rt.h, rt.ptr(self.l), self.line_offsets.ctypes.data_as(vp), rt.ptr(self.vps), self.vp_offsets.ctypes.data_as(vp),
                self.n, index.ctypes.data_as(vp), transforms.ctypes.data_as(vp) if transforms is not None else None, b,
                offsets.ctypes.data_as(vp), self.grid[0], self.grid[1], rt.ptr(l_out), rt.ptr(vp_out), rt.ptr(cell_out),
                rt.ptr(labels)))
            raster_batch_device(rt, l_out if int(offsets[-1]) else None, offsets, self.size, self.alpha, out=rasters)
        if check:
            flags = raster_flags(rt, b)
            if flags.any():
                raise _lib.VpkError("sphere raster: the kernel's buffers were too small for a line of example(s) %s: their "
                                    "rasters are incomplete" % index[np.nonzero(flags)[0]].tolist())
        return {"rasters": rasters, "labels": labels, "l_out": l_out, "vp_out": vp_out, "cell_out": cell_out, "index": index,
                "offsets": offsets, "vp_offsets": vp_offsets, "transforms": transforms}

    def batch(self, iteration, batch, seed=0, augment=None, shuffle=False, check=False):
        """The batch of ``iteration``: (rasters uint8 (B, S, S), labels float32 (B, gh * gw)) as device tensors, ordered on
        the caller's current stream like the trainers' results.  A pure function of the set and of (iteration, batch, seed,
        augment, shuffle): it does not depend on earlier calls."""
        parts = self.batch_parts(iteration, batch, seed, augment, shuffle, check)
        return parts["rasters"], parts["labels"]

    def mean_image(self, chunk=32):
        """float32 (S, S): the mean of the un-augmented rasters of the whole set (transform_param.mean_file), summed in uint32
        on the device in chunks (vpk_trainset_accumulate) and divided once in float64."""
        rt = self.rt
        t = rt.torch
        pixels = self.size * self.size
        count = ctypes.c_int64(0)
        with rt.on_stream():
            total = t.zeros((pixels,), dtype=t.int32, device=rt.tdev)          # the bits of a uint32 sum
        for s in range(0, self.n, int(chunk)):
            idx = np.arange(s, min(self.n, s + int(chunk)), dtype=np.int32)
            rasters = self.batch_parts(0, idx.shape[0], indices=idx, check=True)["rasters"]
            with rt.on_stream():
                rt.check(rt.lib.vpk_trainset_accumulate(rt.h, rt.ptr(rasters), int(idx.shape[0]), pixels, rt.ptr(total),
                                                        ctypes.byref(count)))
        rt.synchronize()
        sums = total.cpu().numpy().view(np.uint32).astype(np.float64)
        return (sums / float(count.value)).astype(np.float32).reshape(self.size, self.size)

    def save_mean(self, path):
        """``mean_image`` as a mean.binaryproto (1, 1, S, S) that caffe_io.read_binaryproto and Caffe read."""
        caffe_io.write_binaryproto(path, self.mean_image().reshape(1, 1, self.size, self.size))


_STATE_LISTS = ("conv_weights", "conv_momentum", "head_weights", "head_momentum")


class Solver(object):
    """The loop of train/solver.prototxt around a trainer (``NetTrainer``, ``StackTrainer``) and a ``TrainSet``: the
    defaults are solver.prototxt's (max_iter, test_iter, test_interval, display, snapshot) and train_val.prototxt's batch
    sizes (TRAIN 5, TEST 100).  The batch of iteration t is ``train_set.batch(t, batch_size, seed, augment, shuffle)``, so
    a restored run continues the data stream where the snapshot left it.  ``log``: a callable for the lines Caffe prints."""

    def __init__(self, trainer, train_set, test_set=None, batch_size=5, test_batch=100, test_iter=288, test_interval=1000,
                 display=100, snapshot=10000, snapshot_prefix=None, max_iter=400000, augment=None, shuffle=False, seed=0,
                 log=print):
        self.trainer, self.train_set, self.test_set = trainer, train_set, test_set
        self.batch_size, self.test_batch, self.test_iter = int(batch_size), int(test_batch), int(test_iter)
        self.test_interval, self.display, self.snapshot_interval = int(test_interval), int(display), int(snapshot)
        self.snapshot_prefix = snapshot_prefix
        self.max_iter = int(max_iter)
        self.augment, self.shuffle, self.seed = augment, bool(shuffle), int(seed)
        self.log = log if log is not None else (lambda line: None)
        self.history = []                       # (event, iteration) of solve(): "test", "display", "snapshot"

    def settings(self):
        return {"batch_size": self.batch_size, "test_batch": self.test_batch, "test_iter": self.test_iter,
                "test_interval": self.test_interval, "display": self.display, "snapshot": self.snapshot_interval,
                "max_iter": self.max_iter, "shuffle": self.shuffle, "seed": self.seed,
                "augment": self.augment.as_dict() if self.augment is not None else None}

    def _iterate(self, iteration):
        rasters, labels = self.train_set.batch(iteration, self.batch_size, self.seed, self.augment, self.shuffle)
        loss, _ = self.trainer.step(rasters, labels)
        return loss

    def step(self, n):
        """n iterations from the trainer's own; returns their losses as one device tensor (n,), nothing is read back."""
        it = self.trainer.iteration
        losses = [self._iterate(it + k) for k in range(int(n))]
        return self.trainer.rt.torch.stack(losses) if losses else None

    def test(self):
        """Caffe's test pass: ``test_iter`` batches of ``test_batch`` examples of the test set from its start, in storage
        order and un-augmented, through ``trainer.evaluate``; the per-batch losses are averaged in float64 on the host.
        Changes no weight."""
        if self.test_set is None:
            raise ValueError("the solver has no test set")
        losses = []
        for k in range(self.test_iter):
            rasters, labels = self.test_set.batch(k, self.test_batch)
            losses.append(self.trainer.evaluate(rasters, labels)[0])
        host = self.trainer.rt.torch.stack(losses).cpu().numpy().astype(np.float64)
        return float(np.mean(host))

    def _test_due(self, it):
        return self.test_set is not None and self.test_interval > 0 and it % self.test_interval == 0

    def _run_test(self, it):
        self.history.append(("test", it))
        self.log("Iteration %d, Testing net: loss = %.9g" % (it, self.test()))

    def solve(self):
        """Runs to ``max_iter`` in Caffe's order (Solver::Step, Solver::Solve): a test pass at iteration 0 and at every
        multiple of test_interval (max_iter included), the loss of every display-th iteration logged (the one read of a
        loss; between displays the losses stay on the device), a snapshot whenever the finished iteration count is a
        multiple of ``snapshot``, and one at the end.  Snapshots need ``snapshot_prefix``."""
        it = self.trainer.iteration
        snapshotted = it
        while it < self.max_iter:
            if self._test_due(it):
                self._run_test(it)
            loss = self._iterate(it)
            if self.display > 0 and it % self.display == 0:
                self.history.append(("display", it))
                self.log("Iteration %d, loss = %.9g" % (it, float(loss)))
            it += 1
            if self.snapshot_prefix is not None and self.snapshot_interval > 0 and it % self.snapshot_interval == 0:
                self.history.append(("snapshot", it))
                self.snapshot()
                snapshotted = it
        if self.snapshot_prefix is not None and snapshotted != it:
            self.history.append(("snapshot", it))
            self.snapshot()
        if self._test_due(it):
            self._run_test(it)
        return it

    def snapshot(self):
        """Writes <prefix>_iter_<N>.solverstate.npz (the trainer's ``state()``, the solver's settings) and, for a trainer
        that has ``save_caffemodel``, <prefix>_iter_<N>.caffemodel.  Returns the solverstate's path.  (Caffe's binary
        .solverstate is not written.)"""
        if self.snapshot_prefix is None:
            raise ValueError("snapshot() needs a snapshot_prefix")
        import json
        state = self.trainer.state()
        base = "%s_iter_%d" % (self.snapshot_prefix, int(state["iteration"]))
        flat = {"iteration": np.int64(state["iteration"]), "trainer_seed": np.uint64(state["seed"]),
                "solver": np.array(json.dumps(self.settings()))}
        for name in _STATE_LISTS:
            flat["n_" + name] = np.int64(len(state[name]))
            for k, a in enumerate(state[name]):
                flat["%s_%d" % (name, k)] = a
        path = base + ".solverstate.npz"
        with open(path, "wb") as fh:
            np.savez(fh, **flat)
        if hasattr(self.trainer, "save_caffemodel"):
            self.trainer.save_caffemodel(base + ".caffemodel")
        return path

    def restore(self, path):
        """Loads a ``snapshot``: the trainer's weights, momentum, iteration and dropout seed, and the solver's data seed.
        The other settings are the constructor's; the snapshot keeps them for the record (``np.load(path)['solver']``)."""
        import json
        with np.load(path) as z:
            state = {"iteration": int(z["iteration"]), "seed": int(z["trainer_seed"])}
            for name in _STATE_LISTS:
                state[name] = [z["%s_%d" % (name, k)] for k in range(int(z["n_" + name]))]
            saved = json.loads(str(z["solver"]))
        self.trainer.load_state(state)
        self.seed = int(saved["seed"])
        return saved
