"""Drop-in for the reference's vp_localisation: expectation_maximisation (vp_localisation.py:168-450) backed by the HIP
EM kernels, and the stand-alone functions around it on the GPU under the reference's names, signatures and defaults.

expectation_maximisation: same name, argument order, defaults, in-place normalisation of ``l`` and result keys (including
'distribution', the PDF tuple of the last E-step); `distance_measure` other than "angle" raises AssertionError as at :203.

Line geometry (vpk_line_similarity_batch, vpk_line_rating_batch; include/vpk.h): calc_lsim (:87-108), line_rating_knn
(:34-72), lines_angles (:765-776) and line_length (:761) take and return NumPy arrays and leave ``lp`` untouched;
calc_lsim_batch and line_geometry_batch take many images at once and return device tensors.  The EM itself calls the pair
functions with sigma = 1 and k2 = 4 (:178, :230); the defaults here are the reference functions' own (0.1 and 3).

Thin mirrors of entry points the EM's unit tests already use: find_initial_vps (:111-165, vpk_init_vps), weight_matrix
(:515-524, vpk_weight_matrix) and calc_new_vanishing_point (:453-479, vpk_mstep).

Not here: calc_vp_line_counts, split_best_vp and merge_vps (they live inside the EM workgroup; kernels.line_counts and
kernels.cluster2 are their fine-grained entries), the scalar pair helpers (lines_similarity, lines_proximity,
lines_points_cosangle, line_distance_closest, line_segment_point_distance: device functions of csrc/line_device.hpp) and
the distance measures other than "angle".  There is no host fallback: without the library and a GPU every call but
line_length raises."""
import numpy as np

from . import em as _em
from . import kernels as _kernels
from ._lib import host_i64


def expectation_maximisation(l, lp, cnn_response, num_iter=100, sphere_image=None, init_vp=None,
                             do_merge=True, do_split=True, do_iterations=True, distance_measure="angle",
                             use_weights=True, wbias=1, num_init_vp=25, split_merge_freq=10,
                             merge_thresh=1e-3, outlier_thresh=1.96 ** 2, final_convergence=5e-3,
                             s_thresh=1e-200, num_min_lines=3, device=0, want_metric=True, return_distribution=True):
    if sphere_image is None:
        raise TypeError("sphere_image is required (the reference dereferences it at vp_localisation.py:113)")
    scene = {"l": l, "lp": lp, "cnn_response": cnn_response, "sphere_image": sphere_image,
             "init_vp": init_vp}
    # 'distribution' is the reference's probability_functions.PDF tuple (:441), as in the reference's result
    res = _em.em_batch([scene], device=device, want_metric=want_metric, want_distribution=return_distribution,
                       num_iter=num_iter,
                       do_merge=do_merge, do_split=do_split, do_iterations=do_iterations,
                       distance_measure=distance_measure, use_weights=use_weights, wbias=wbias,
                       num_init_vp=num_init_vp, split_merge_freq=split_merge_freq,
                       merge_thresh=merge_thresh, outlier_thresh=outlier_thresh,
                       final_convergence=final_convergence, s_thresh=s_thresh,
                       num_min_lines=num_min_lines)[0]
    status = res.pop("status")
    l_norm = res.pop("l")
    if isinstance(l, np.ndarray) and l.dtype == np.float64:
        l[...] = l_norm                       # the reference normalises the caller's array (:185-186)
    if status == 2:                           # np.vstack([]) at vp_localisation.py:165
        raise ValueError("need at least one array to concatenate")
    return res


# ---- line geometry -------------------------------------------------------------------------------------------------------
K1_MAX = 16      # capacity of the rating kernel's neighbour lists (csrc/line_device.hpp: LR_K)
MAT_ALIGN = 16   # matrices of calc_lsim_batch start at multiples of 16 elements: whole 128-byte lines where N allows


def _runtime(device):
    from .runtime import get_runtime
    return get_runtime(device)


def _check_sigma(sigma):
    sigma = float(sigma)
    if not sigma > 0:
        raise ValueError("sigma must be positive (got %r)" % sigma)
    return sigma


def _check_knn(k1, k2):
    k1, k2 = int(k1), int(k2)
    if k1 < 1 or k2 < 1:
        raise ValueError("k1 and k2 must be at least 1 (got k1 = %d, k2 = %d)" % (k1, k2))
    if k1 > K1_MAX:
        raise ValueError("k1 = %d: at most %d neighbours are supported -- up to 16 elements NumPy's argsort is an insertion "
                         "sort, beyond that the reference's own order among equal cosines is that of an unstable sort"
                         % (k1, K1_MAX))
    if k2 > k1:
        raise ValueError("k2 = %d exceeds k1 = %d: the reference indexes past its k1 neighbours there (IndexError at "
                         "vp_localisation.py:63)" % (k2, k1))
    return k1, k2


def _check_lp(lp):
    lp = np.asarray(lp)
    if lp.ndim != 2 or lp.shape[1] != 4:
        raise ValueError("lp must be (N, 4) segment end points (got shape %r)" % (lp.shape,))
    return lp


def _is_device_pair(lps):
    return isinstance(lps, tuple) and len(lps) == 2 and hasattr(lps[0], "data_ptr")


def _check_batch(lps):
    """The image sizes' offsets (host int64) of ``lps``; raises before the GPU is touched."""
    if _is_device_pair(lps):
        d_lp, offsets = lps
        offsets = host_i64(offsets)
        if d_lp.dim() != 2 or d_lp.shape[1] != 4:
            raise ValueError("the device form of lps is a (sum N, 4) tensor and its offsets")
        if offsets.ndim != 1 or offsets.shape[0] < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any() or \
                offsets[-1] != d_lp.shape[0]:
            raise ValueError("offsets must rise from 0 to the number of lines (%d)" % d_lp.shape[0])
        return offsets
    sizes = [_check_lp(a).shape[0] for a in lps]
    return np.concatenate(([0], np.cumsum(sizes, dtype=np.int64))).astype(np.int64)


def _lines_on_device(rt, lps):
    """(sum N, 4) float64 device tensor of a batch; the caller's arrays are only read."""
    t = rt.torch
    if _is_device_pair(lps):
        return lps[0].to(device=rt.tdev, dtype=t.float64).contiguous()
    arrs = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 4) for a in lps]
    cat = np.concatenate(arrs) if arrs else np.zeros((0, 4))
    return t.from_numpy(cat).to(rt.tdev)


def _off_ptr(a):
    import ctypes
    return a.ctypes.data_as(ctypes.c_void_p)


def _rating(lps, k1, k2, sigma, want, device):
    """vpk_line_rating_batch: (lscore, langle, llen) device tensors, None where ``want`` says so, and the offsets."""
    k1, k2 = _check_knn(k1, k2)
    sigma = _check_sigma(sigma)
    offsets = _check_batch(lps)
    rt = _runtime(device)
    t = rt.torch
    total = int(offsets[-1])
    with rt.on_stream():
        d_lp = _lines_on_device(rt, lps)
        outs = [t.empty((total,), dtype=t.float64, device=rt.tdev) if w else None for w in want]
        rt.check(rt.lib.vpk_line_rating_batch(rt.h, offsets.shape[0] - 1, _off_ptr(offsets), rt.ptr(d_lp), k1, k2, sigma,
                                              rt.ptr(outs[0]), rt.ptr(outs[1]), rt.ptr(outs[2])))
    rt.synchronize()
    return outs, offsets


def calc_lsim_batch(lps, sigma=0.1, device=0):
    """calc_lsim for many images in one launch.  ``lps``: a list of (N_b, 4) arrays, or a pair (device tensor (sum N, 4)
    float64, host offsets).  Returns a list of (N_b, N_b) float64 device tensors, views into one allocation."""
    sigma = _check_sigma(sigma)
    offsets = _check_batch(lps)
    sizes = np.diff(offsets)
    mat = np.zeros(offsets.shape[0], dtype=np.int64)
    np.cumsum((sizes * sizes + MAT_ALIGN - 1) // MAT_ALIGN * MAT_ALIGN, out=mat[1:])
    rt = _runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_lp = _lines_on_device(rt, lps)
        buf = t.empty((int(mat[-1]),), dtype=t.float64, device=rt.tdev)
        rt.check(rt.lib.vpk_line_similarity_batch(rt.h, sizes.shape[0], _off_ptr(offsets), rt.ptr(d_lp), sigma, _off_ptr(mat),
                                                  rt.ptr(buf)))
    rt.synchronize()
    return [buf[int(m):int(m) + int(n) * int(n)].view(int(n), int(n)) for m, n in zip(mat[:-1], sizes)]


def line_geometry_batch(lps, k1=10, k2=3, sigma=1, device=0):
    """line_rating_knn, lines_angles and line_length for many images in one launch, without an N x N matrix.  ``lps`` as in
    calc_lsim_batch.  Returns (lscore, langle, llen, offsets): three float64 device tensors of sum N elements and the host
    int64 offsets (image b: [offsets[b], offsets[b + 1]))."""
    (lscore, langle, llen), offsets = _rating(lps, k1, k2, sigma, (True, True, True), device)
    return lscore, langle, llen, offsets


def calc_lsim(lp, sigma=0.1, device=0):
    """calc_lsim (:87-108): the symmetric (N, N) similarity matrix, zero diagonal."""
    _check_sigma(sigma)
    if _check_lp(lp).shape[0] == 0:
        raise ValueError("need at least one array to stack")       # np.stack([]) at :93
    return calc_lsim_batch([lp], sigma=sigma, device=device)[0].cpu().numpy()


def line_rating_knn(lp, k1=10, k2=3, sigma=1, device=0):
    """line_rating_knn (:34-72): the (N,) scores, before any clip.  k1 <= 16 and k2 <= k1, else ValueError."""
    _check_knn(k1, k2)
    _check_sigma(sigma)
    if _check_lp(lp).shape[0] == 0:
        raise ValueError("need at least one array to stack")       # np.stack([]) at :45
    return _rating([lp], k1, k2, sigma, (True, False, False), device)[0][0].cpu().numpy()


def lines_angles(lp, device=0):
    """lines_angles (:765-776): every line's angle against the x axis, folded into [0, pi / 2]."""
    if _check_lp(lp).shape[0] == 0:
        return np.zeros(0)
    return _rating([lp], 1, 1, 1.0, (False, True, False), device)[0][1].cpu().numpy()


def line_length(lp):
    """line_length (:761) of ONE segment (x1, y1, x2, y2), on the host as in the reference."""
    return np.linalg.norm(lp[0:2] - lp[2:4], ord=2)


# ---- thin mirrors of the EM's fine-grained entry points -------------------------------------------------------------------
def find_initial_vps(sphere_image, cnn_response, num_max, device=0):
    """find_initial_vps (:111-165): the (M, 3) initial VPs; none at all raises np.vstack([])'s ValueError (:165)."""
    vps, _ = _kernels.init_vps(cnn_response, sphere_image, num_max=num_max, device=device)
    if vps.shape[0] == 0:
        raise ValueError("need at least one array to concatenate")
    return vps


def weight_matrix(p_vl, lweight, lsim, bias=0.001, device=0):
    """weight_matrix (:515-524): p_vl (M, N), lweight (N,), lsim (N, N) -> w (M, N)."""
    return _kernels.weight_matrix(p_vl, lweight, lsim, bias=bias, device=device)


def calc_new_vanishing_point(l, w, device=0):
    """calc_new_vanishing_point (:453-479) for one weight row: the unit VP, or None where the reference returns None
    (no weights, :456-457; all weights zero, :459-460)."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.size == 0:
        return None
    vp, valid = _kernels.mstep(l, w[None, :], device=device)
    return vp[0] if valid[0] else None
