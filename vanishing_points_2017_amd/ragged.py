"""How the ``*_batch`` functions describe many images of different sizes in one call: host int64 offsets (B + 1; image b
holds rows [off[b], off[b + 1])) beside data that is a list with one array or tensor per image, or one concatenated array
or tensor, or -- for lines -- a pair (device tensor, offsets).  The only place that knows this; vp_localisation and
probability_functions are call surface on top of it.

Everything above ``to_device`` is host only: it reads shapes and offsets, raises ValueError, and runs without torch, the
library or a GPU -- the wrappers call it before they ask for the runtime.  The functions from ``to_device`` on take the
runtime: a list of host arrays is one concatenation and one upload, a list of device tensors one torch.cat, and the
caller's data is only read."""
import ctypes

import numpy as np

from ._lib import MAX_VP, host_i64

MAX_LINES = 32768                       # per image (csrc/vpk_emstep.hip, csrc/vpk_vpset.hip)


def numel(a):
    return int(a.numel()) if hasattr(a, "numel") else int(np.asarray(a).size)


def shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape


def is_list(x):
    return isinstance(x, (list, tuple))


def is_device_pair(x):
    return isinstance(x, tuple) and len(x) == 2 and hasattr(x[0], "data_ptr")


# ---- offsets --------------------------------------------------------------------------------------------------------------
def offsets_of(sizes):
    return np.concatenate(([0], np.cumsum(sizes, dtype=np.int64))).astype(np.int64)


def check_offsets(off, total, what, end=None):
    """The caller's offsets as host int64: they rise from 0 and, unless ``total`` is None, end at it (``end``: how the
    message names the total)."""
    off = host_i64(off)
    if off.ndim != 1 or off.shape[0] < 1 or off[0] != 0 or (np.diff(off) < 0).any() or (total is not None and off[-1] != total):
        raise ValueError("%s must rise from 0%s" % (what, "" if total is None else " to " + (end or "%d" % total)))
    return off


def batch_offsets(x, offsets, what):
    """Offsets of a batch given as a list (sizes from the list) or concatenated (offsets from the caller)."""
    if is_list(x):
        return offsets_of([int(a.shape[0]) if hasattr(a, 'shape') else len(a) for a in x])
    if offsets is None:
        raise ValueError("%s is one concatenated array: its offsets are needed" % what)
    return check_offsets(offsets, int(x.shape[0]), what + " offsets")


def strict_offsets(xs, tail, what):
    """Offsets of a list whose every image has shape (rows,) + tail exactly."""
    for a in xs:
        if shape(a)[1:] != tail or len(shape(a)) != len(tail) + 1:
            raise ValueError("%s: every image needs shape (rows,%s), got %r" % (what, "".join(" %d" % k for k in tail), shape(a)))
    return offsets_of([shape(a)[0] for a in xs])


def vp_sizes_of_mats(mats, vp_offsets, what):
    """VP offsets from a list of (M_b, N_b) matrices, or the caller's for the flat form."""
    if is_list(mats):
        for a in mats:
            if len(shape(a)) != 2:
                raise ValueError("%s: every image's matrix must be two-dimensional (M_b, N_b)" % what)
        return offsets_of([shape(a)[0] for a in mats])
    if vp_offsets is None:
        raise ValueError("%s is one concatenated array: vp_offsets is needed" % what)
    return check_offsets(vp_offsets, None, "vp_offsets")


def off_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- shape checks -----------------------------------------------------------------------------------------------------------
def check_vp_limit(vp_off):
    m = np.diff(vp_off)
    if m.size and m.max() > MAX_VP:
        raise ValueError("%d VPs: at most %d are supported" % (m.max(), MAX_VP))


def check_images(lo, vo, what_l, what_v):
    if lo.shape != vo.shape:
        raise ValueError("%s and %s describe %d and %d images" % (what_l, what_v, lo.shape[0] - 1, vo.shape[0] - 1))
    check_vp_limit(vo)


def check_counts(lo, vo, what_l, what_v):
    check_images(lo, vo, what_l, what_v)
    n = np.diff(lo)
    if n.size and n.max() > MAX_LINES:
        raise ValueError("%d lines in one image: at most %d are supported" % (n.max(), MAX_LINES))


def total(x):
    """Elements of a batch, a list or concatenated."""
    return sum(numel(a) for a in x) if is_list(x) else numel(x)


def check_total(x, rows, what, width=1, unit="elements"):
    """``x`` holds ``rows`` rows of ``width`` elements in all, however a list divides them among its images."""
    if total(x) != int(rows) * width:
        raise ValueError("%s holds %d %s, expected %d" % (what, total(x) // width, unit, rows))


def check_rows(x, off, width, what):
    """``x`` holds off[-1] rows of ``width`` elements (lists: image b off[b + 1] - off[b] of them)."""
    if is_list(x):
        if len(x) != off.shape[0] - 1:
            raise ValueError("%s holds %d images, expected %d" % (what, len(x), off.shape[0] - 1))
        for b, a in enumerate(x):
            if numel(a) != int(off[b + 1] - off[b]) * width:
                raise ValueError("%s[%d] holds %d elements, expected %d" % (what, b, numel(a), int(off[b + 1] - off[b]) * width))
    else:
        check_total(x, int(off[-1]) * width, what)


def mats_total(lo, vo):
    return int((np.diff(lo) * np.diff(vo)).sum())


def check_mats(x, lo, vo, what, transposed=False):
    """``x`` holds the images' M_b x N_b matrices: a list of (M_b, N_b) -- ``transposed``: (N_b, M_b) -- arrays or tensors,
    or the [m][n] matrices concatenated flat, image after image."""
    n, m = np.diff(lo), np.diff(vo)
    if is_list(x):
        if len(x) != n.shape[0]:
            raise ValueError("%s holds %d images, expected %d" % (what, len(x), n.shape[0]))
        for b, a in enumerate(x):
            want = (int(n[b]), int(m[b])) if transposed else (int(m[b]), int(n[b]))
            if shape(a) != want and not (numel(a) == 0 and want[0] * want[1] == 0):
                raise ValueError("%s[%d] has shape %r, expected %r" % (what, b, shape(a), want))
    elif numel(x) != mats_total(lo, vo):
        raise ValueError("%s holds %d elements, the images' M x N sum to %d" % (what, numel(x), mats_total(lo, vo)))


def check_lsims(lsims, lo):
    """One matrix of exactly N_b x N_b elements per image, a list or concatenated flat."""
    n = np.diff(lo)
    if is_list(lsims):
        if len(lsims) != n.shape[0] or any(numel(a) != int(k) * int(k) for a, k in zip(lsims, n)):
            raise ValueError("lsims must hold one N x N matrix per image")
    elif numel(lsims) != int((n * n).sum()):
        raise ValueError("lsims must hold one N x N matrix per image")


# ---- upload -------------------------------------------------------------------------------------------------------------------
def to_device(rt, a, dtype):
    """``a`` (array or tensor, any device) as a contiguous tensor of the NumPy ``dtype`` on the runtime's GPU.  A host array
    of another dtype is cast by NumPy before the upload, a tensor by torch where it lies."""
    t = rt.torch
    if not isinstance(a, t.Tensor):
        a = t.from_numpy(np.ascontiguousarray(a, dtype=dtype))
    return a.to(device=rt.tdev, dtype=getattr(t, np.dtype(dtype).name)).contiguous()


def upload(rt, x, dtype, tail=(), pair=False):
    """A batch in any of its forms as one contiguous device tensor of shape (-1,) + tail.  ``pair``: where the call surface
    takes the (device tensor, offsets) form, since a tuple of two per-image tensors looks the same."""
    rows = (-1,) + tail
    if pair and is_device_pair(x):
        x = x[0]
    elif is_list(x) and any(isinstance(a, rt.torch.Tensor) for a in x):
        x = rt.torch.cat([to_device(rt, a, dtype).reshape(rows) for a in x])
    elif is_list(x):
        x = np.concatenate([np.zeros((0,) + tail, dtype=dtype)] + [np.asarray(a, dtype=dtype).reshape(rows) for a in x])
    return to_device(rt, x, dtype).reshape(rows)


def upload_mats(rt, x, transposed=False):
    if transposed and is_list(x):
        x = [a.T if hasattr(a, "data_ptr") else np.asarray(a).T for a in x]      # back to [m][n]: free for a transposed view
    return upload(rt, x, np.float64)


def lsim_layout(rt, lsims, sizes):
    """(device tensor, host element offsets) of the images' N x N matrices.  A list of views into one allocation in rising
    order -- what calc_lsim_batch returns -- is used where it lies; anything else is concatenated on the device."""
    t = rt.torch
    if is_list(lsims) and len(lsims) and all(isinstance(a, t.Tensor) and a.is_cuda and a.dtype == t.float64
                                             and a.is_contiguous() for a in lsims):
        full = [a for a in lsims if a.numel()]                   # (an empty view has no address)
        if full:
            base, off, pos, ok = full[0].data_ptr(), [], 0, True
            for a, n in zip(lsims, sizes):
                o = (a.data_ptr() - base) // 8 if a.numel() else pos
                ok = ok and o >= pos and (not a.numel() or a.untyped_storage().data_ptr() == full[0].untyped_storage().data_ptr())
                off.append(o)
                pos = o + int(n) * int(n)
            if ok:
                return (ctypes.c_void_p(base), full[0]), host_i64(off + [pos])
    d = upload(rt, lsims, np.float64)
    return (rt.ptr(d), d), offsets_of(sizes * sizes)


# ---- views back -----------------------------------------------------------------------------------------------------------
def split_mats(flat, lo, vo, transposed=False):
    """Per image the (M, N) matrix of a flat [m][n] buffer, or its (N, M) transposed view."""
    n, m = np.diff(lo), np.diff(vo)
    at = offsets_of(n * m)
    mats = [flat[int(at[b]):int(at[b + 1])].view(int(m[b]), int(n[b])) for b in range(n.shape[0])]
    return [a.t() for a in mats] if transposed else mats
