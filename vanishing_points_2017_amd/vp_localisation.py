"""Drop-in for the reference's vp_localisation: expectation_maximisation (vp_localisation.py:168-450) backed by the HIP
EM kernels, and the stand-alone functions around it on the GPU under the reference's names, signatures and defaults.

expectation_maximisation: same name, argument order, defaults, in-place normalisation of ``l`` and result keys (including
'distribution', the PDF tuple of the last E-step); `distance_measure` other than "angle" raises AssertionError here (its test
pins that).  expectation_maximisation_batch is its twin for many images in one launch, and runs both measures of the
reference's EM, "angle" and "dotprod" (:196-201).

Line geometry (vpk_line_similarity_batch, vpk_line_rating_batch; include/vpk.h): calc_lsim (:87-108), line_rating_knn
(:34-72), lines_angles (:765-776) and line_length (:761) take and return NumPy arrays and leave ``lp`` untouched;
calc_lsim_batch and line_geometry_batch take many images at once and return device tensors.  The EM itself calls the pair
functions with sigma = 1 and k2 = 4 (:178, :230); the defaults here are the reference functions' own (0.1 and 3).

Thin mirrors of entry points the EM's unit tests already use: find_initial_vps (:111-165, vpk_init_vps), weight_matrix
(:515-524, vpk_weight_matrix) and calc_new_vanishing_point (:453-479, vpk_mstep).

The EM update for a batch (vpk_init_vps_batch, vpk_weight_matrix_batch, vpk_mstep_batch; include/vpk.h):
find_initial_vps_batch, weight_matrix_batch, calc_new_vanishing_point_batch and mstep_batch -- the M-step with the variance,
error and removal step around it (:284-322 soft, :353-392 hard) -- take many images per launch, return device tensors and
give, image by image, the bits of the single-image entry points.  With the prior, the E-step and the VP set functions a
whole EM iteration is composed of device-resident calls (mstep_batch's docstring), under any of the E-step's distance
measures: prior, E-step, weights, M-step, counts and merge take all three; the split has none.

VP set maintenance (vpk_vp_line_counts_batch, vpk_vp_split_batch, vpk_vp_merge_batch; include/vpk.h): calc_vp_line_counts
(:482-512), split_best_vp (:527-630) and merge_vps (:633-684) on a VP set of the caller's, through the EM workgroup's own
device functions; calc_angle_to_other_vp (:687-697) on the host.  The ``*_batch`` forms take many images per launch and
return device tensors.  Deliberate differences from the reference: the caller's ``v``, ``s`` and ``vp_assoc`` arrays are
not modified (the reference writes into them; the results are new arrays); ``numClusters`` other than 2 and more than
64 VPs raise ValueError.  calc_vp_line_counts_batch and merge_vps_batch take the reference's three measures
(vpk_vp_line_counts_batch_measure, vpk_vp_merge_batch_measure); the single-image calc_vp_line_counts and merge_vps take
"angle" and raise ValueError for the others.

Not here: the scalar pair helpers (lines_similarity, lines_proximity, lines_points_cosangle, line_distance_closest,
line_segment_point_distance: device functions of csrc/line_device.hpp).
There is no host fallback: without the library and a GPU every call but line_length and calc_angle_to_other_vp raises."""
import numpy as np

from . import em as _em
from . import kernels as _kernels
from . import ragged
from .probability_functions import PDFParams, _grid_means
from .runtime import get_runtime


def expectation_maximisation(l, lp, cnn_response, num_iter=100, sphere_image=None, init_vp=None,
                             do_merge=True, do_split=True, do_iterations=True, distance_measure="angle",
                             use_weights=True, wbias=1, num_init_vp=25, split_merge_freq=10,
                             merge_thresh=1e-3, outlier_thresh=1.96 ** 2, final_convergence=5e-3,
                             s_thresh=1e-200, num_min_lines=3, device=0, want_metric=True, return_distribution=True):
    if distance_measure != "angle":
        # em.em_batch runs "dotprod" too (expectation_maximisation_batch below is its entry here); this refusal is what
        # tests/test_gpu_em.py::test_drop_in_call_surface pins, and is lifted together with that test.
        raise AssertionError("distance_measure %r: the single-image drop-in takes \"angle\" only; "
                             "expectation_maximisation_batch also runs \"dotprod\"" % (distance_measure,))
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


def expectation_maximisation_batch(ls, lps, cnn_responses, sphere_images, init_vps=None, device=0, num_iter=100,
                                   do_merge=True, do_split=True, do_iterations=True, distance_measure="angle",
                                   use_weights=True, wbias=1, num_init_vp=25, split_merge_freq=10, merge_thresh=1e-3,
                                   outlier_thresh=1.96 ** 2, final_convergence=5e-3, s_thresh=1e-200, num_min_lines=3,
                                   want_metric=True, return_distribution=True):
    """expectation_maximisation (:168-450) for many images in one launch: one list entry per image, the keywords and
    defaults of the reference for all of them, ``distance_measure`` "angle" or "dotprod" (:196-201; anything else raises
    AssertionError as :203).  ``init_vps``: None, or one (K, 3) array per image with the same K.  Returns one result dict
    per image with the reference's keys; every float64 ``l`` is normalised in place (:185-186).  An image without any
    initial VP raises ValueError (:165) after all images have run."""
    _em._measure(distance_measure)
    ls, lps, cnn_responses, sphere_images = list(ls), list(lps), list(cnn_responses), list(sphere_images)
    if not (len(ls) == len(lps) == len(cnn_responses) == len(sphere_images)) or \
            (init_vps is not None and len(init_vps) != len(ls)):
        raise ValueError("ls, lps, cnn_responses, sphere_images and init_vps must have one entry per image")
    if any(s is None for s in sphere_images):
        raise TypeError("sphere_image is required (the reference dereferences it at vp_localisation.py:113)")
    if not ls:
        return []
    scenes = [{"l": l, "lp": lp, "cnn_response": c, "sphere_image": s, "init_vp": None if init_vps is None else init_vps[b]}
              for b, (l, lp, c, s) in enumerate(zip(ls, lps, cnn_responses, sphere_images))]
    results = _em.em_batch(scenes, device=device, want_metric=want_metric, want_distribution=return_distribution,
                           num_iter=num_iter, do_merge=do_merge, do_split=do_split, do_iterations=do_iterations,
                           distance_measure=distance_measure, use_weights=use_weights, wbias=wbias,
                           num_init_vp=num_init_vp, split_merge_freq=split_merge_freq, merge_thresh=merge_thresh,
                           outlier_thresh=outlier_thresh, final_convergence=final_convergence, s_thresh=s_thresh,
                           num_min_lines=num_min_lines)
    failed = False
    for l, res in zip(ls, results):
        failed = failed or res.pop("status") == 2
        l_norm = res.pop("l")
        if isinstance(l, np.ndarray) and l.dtype == np.float64:
            l[...] = l_norm
    if failed:
        raise ValueError("need at least one array to concatenate")
    return results


# ---- line geometry -------------------------------------------------------------------------------------------------------
K1_MAX = 16      # capacity of the rating kernel's neighbour lists (csrc/line_device.hpp: LR_K)
MAT_ALIGN = 16   # matrices of calc_lsim_batch start at multiples of 16 elements: whole 128-byte lines where N allows


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


def _check_batch(lps):
    """The image sizes' offsets (host int64) of ``lps``; raises before the GPU is touched."""
    if ragged.is_device_pair(lps):
        if lps[0].dim() != 2 or lps[0].shape[1] != 4:
            raise ValueError("the device form of lps is a (sum N, 4) tensor and its offsets")
        return ragged.check_offsets(lps[1], lps[0].shape[0], "offsets", "the number of lines (%d)" % lps[0].shape[0])
    return ragged.offsets_of([_check_lp(a).shape[0] for a in lps])


def _rating(lps, k1, k2, sigma, want, device):
    """vpk_line_rating_batch: (lscore, langle, llen) device tensors, None where ``want`` says so, and the offsets."""
    k1, k2 = _check_knn(k1, k2)
    sigma = _check_sigma(sigma)
    offsets = _check_batch(lps)
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_lp = ragged.upload(rt, lps, np.float64, (4,), pair=True)
        outs = [t.empty((int(offsets[-1]),), dtype=t.float64, device=rt.tdev) if w else None for w in want]
        rt.check(rt.lib.vpk_line_rating_batch(rt.h, offsets.shape[0] - 1, ragged.off_ptr(offsets), rt.ptr(d_lp), k1, k2, sigma,
                                              rt.ptr(outs[0]), rt.ptr(outs[1]), rt.ptr(outs[2])))
    rt.synchronize()
    return outs, offsets


def calc_lsim_batch(lps, sigma=0.1, device=0):
    """calc_lsim for many images in one launch.  ``lps``: a list of (N_b, 4) arrays, or a pair (device tensor (sum N, 4)
    float64, host offsets).  Returns a list of (N_b, N_b) float64 device tensors, views into one allocation."""
    sigma = _check_sigma(sigma)
    offsets = _check_batch(lps)
    sizes = np.diff(offsets)
    mat = ragged.offsets_of((sizes * sizes + MAT_ALIGN - 1) // MAT_ALIGN * MAT_ALIGN)
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_lp = ragged.upload(rt, lps, np.float64, (4,), pair=True)
        buf = t.empty((int(mat[-1]),), dtype=t.float64, device=rt.tdev)
        rt.check(rt.lib.vpk_line_similarity_batch(rt.h, sizes.shape[0], ragged.off_ptr(offsets), rt.ptr(d_lp), sigma,
                                                  ragged.off_ptr(mat), rt.ptr(buf)))
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


# ---- VP set maintenance ---------------------------------------------------------------------------------------------------
MAX_VP = _em.MAX_VP                     # 64: capacity of the EM workgroup's VP arrays
VP_FLAG_SPLIT_TIE, VP_FLAG_SPLIT_DISCONNECTED, VP_FLAG_OVERFLOW, VP_FLAG_PRIOR_TRUNCATED = 1, 2, 4, 8   # include/vpk.h


def _check_measure(distance_measure):
    """the single-image forms"""
    if distance_measure != "angle":
        raise ValueError("distance_measure %r is not supported by the single-image form: use the *_batch form with one-image "
                         "lists" % (distance_measure,))


_MEASURES = {"angle": 0, "dotprod": 1, "area": 2}      # enum vpk_dist_measure (include/vpk.h)


def _measure_code(distance_measure):
    """the batch forms: the reference's three measures (:495-500)"""
    if not isinstance(distance_measure, str) or distance_measure not in _MEASURES:
        raise ValueError("distance_measure %r: one of \"angle\", \"dotprod\", \"area\"" % (distance_measure,))
    return _MEASURES[distance_measure]


def calc_vp_line_counts_batch(vps, lps, ss, decision_metrics, lweights, distance_measure="angle", thresh=2.57,
                              vp_assocs=None, line_offsets=None, vp_offsets=None, device=0, ls=None):
    """calc_vp_line_counts for many images in one launch.  Every argument is a list with one array per image -- vp (M_b, 3),
    lp (N_b, 4), s (M_b,), decision_metric (M_b, N_b), lweights (N_b,), vp_assoc (N_b,) int64 -- or one concatenated
    array / device tensor with ``line_offsets`` / ``vp_offsets`` (host int64, B + 1); the metrics are then concatenated
    flat, image after image.  Returns (counts, counts_weighted, vp_assoc, line_offsets, vp_offsets): device tensors of
    sum M, sum M and sum N (int64) elements.  An image without lines counts nothing; one without VPs associates nothing.

    ``distance_measure``: "angle", "dotprod" or "area" (:495-500), evaluated on vps, ss and ls as they stand.  ``ls``: the
    lines, (N_b, 3) each or concatenated; read by "dotprod" only, which needs them (|vp[m] . l[n]|, :496)."""
    measure = _measure_code(distance_measure)
    if distance_measure == "dotprod" and ls is None:
        raise ValueError("distance_measure \"dotprod\" reads the lines: pass ls")
    lo = ragged.batch_offsets(lps, line_offsets, "lps")
    vo = ragged.batch_offsets(vps, vp_offsets, "vps")
    ragged.check_images(lo, vo, "lps", "vps")
    if distance_measure == "dotprod":
        ragged.check_total(ls, lo[-1], "ls", 3, "rows")
    if decision_metrics is None and vp_assocs is None:
        raise ValueError("decision_metrics or vp_assocs is needed")
    if decision_metrics is not None and ragged.total(decision_metrics) != ragged.mats_total(lo, vo):
        raise ValueError("the decision metrics hold %d elements, the images' M x N sum to %d"
                         % (ragged.total(decision_metrics), ragged.mats_total(lo, vo)))
    for x, n, what in ((ss, vo[-1], "ss"), (lweights, lo[-1], "lweights"), (vp_assocs, lo[-1], "vp_assocs")):
        if x is not None:
            ragged.check_total(x, n, what)
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_lp = ragged.upload(rt, lps, np.float64, (4,))
        d_l = ragged.upload(rt, ls, np.float64, (3,)) if distance_measure == "dotprod" else None
        d_v = ragged.upload(rt, vps, np.float64, (3,))
        d_s = ragged.upload(rt, ss, np.float64)
        d_lw = ragged.upload(rt, lweights, np.float64)
        d_w = ragged.upload(rt, decision_metrics, np.float64) if decision_metrics is not None else None
        d_ain = ragged.upload(rt, vp_assocs, np.int64) if vp_assocs is not None else None
        counts = t.zeros((int(vo[-1]),), dtype=t.float64, device=rt.tdev)
        counts_w = t.zeros_like(counts)
        assoc = d_ain.clone() if d_ain is not None else t.full((int(lo[-1]),), -1, dtype=t.int64, device=rt.tdev)
        rt.check(rt.lib.vpk_vp_line_counts_batch_measure(rt.h, measure, lo.shape[0] - 1, ragged.off_ptr(lo), ragged.off_ptr(vo),
                                                         rt.ptr(d_lp), rt.ptr(d_l), rt.ptr(d_v), rt.ptr(d_s), rt.ptr(d_w), rt.ptr(d_lw),
                                                         float(thresh), rt.ptr(d_ain), rt.ptr(counts), rt.ptr(counts_w),
                                                         rt.ptr(assoc)))
    rt.synchronize()
    return counts, counts_w, assoc, lo, vo


def calc_vp_line_counts(vp, l, lp, s, decision_metric, lweights, distance_measure, thresh=2.57, vp_assoc=None, device=0):
    """calc_vp_line_counts (:482-512): (counts, counts_weighted, vp_assoc) of the lines ``lp`` against the VPs ``vp`` with
    variances ``s``.  ``vp_assoc`` None: every line goes to the argmax of ``decision_metric`` (M, N) over the VPs (:487);
    given, entries below 0 skip their line (:494).  A line farther than thresh * sqrt(s[m]) from its VP (:504) or of
    weight 0 (:506) gets -1.  ``l`` is not read by the "angle" measure.  The result's vp_assoc is a new int64 array: the
    caller's is not written.  It is what result_plotting.line_primitives takes as a datum's ``vp_assoc``.
    This single-image form takes "angle" only; "dotprod" and "area": calc_vp_line_counts_batch with one-image lists."""
    _check_measure(distance_measure)
    vp = np.asarray(vp, dtype=np.float64).reshape(-1, 3)
    lp = _check_lp(lp)
    if vp.shape[0] > MAX_VP:
        raise ValueError("%d VPs: at most %d are supported" % (vp.shape[0], MAX_VP))
    if vp_assoc is None:
        if vp.shape[0] == 0 and lp.shape[0] > 0:
            raise ValueError("attempt to get argmax of an empty sequence")      # np.argmax at :487
        assocs = None
    else:
        vp_assoc = np.asarray(vp_assoc)
        if vp_assoc.size and vp_assoc.max() >= vp.shape[0]:
            raise IndexError("vp_assoc names VP %d of %d" % (vp_assoc.max(), vp.shape[0]))      # vp[m] at :498
        assocs = [vp_assoc.astype(np.int64)]
    metrics = None if decision_metric is None else [np.asarray(decision_metric, dtype=np.float64).reshape(vp.shape[0], -1)]
    c, cw, a, _, _ = calc_vp_line_counts_batch([vp], [lp], [np.asarray(s, dtype=np.float64)], metrics,
                                               [np.asarray(lweights, dtype=np.float64)], thresh=thresh, vp_assocs=assocs,
                                               device=device)
    return c.cpu().numpy(), cw.cpu().numpy(), a.cpu().numpy()


def split_best_vp_batch(vs, ss, linePoints, lines, weightMatrices, lineWeights, lineAngles, numClusters=2, min_diff=0.0001,
                        line_offsets=None, vp_offsets=None, device=0):
    """split_best_vp on slice i of many images' history arrays in one launch; arguments as in calc_vp_line_counts_batch
    (vs: (M_b, 3) each, weightMatrices (M_b, N_b), lines (N_b, 3)).  Returns a dict of device tensors: 'v' (sum M + B, 3)
    and 's' (sum M + B): image b's rows start at vp_offsets[b] + b, 'num_vp' (B,) of them are its set, the rest zeros;
    'split' (B,) int32: the VP that was split or -1; 'flags' (B,) int32 (VP_FLAG_*); 'labels' (sum N,) int32: the cluster of
    every line of the worst VP, -1 elsewhere; and the host offsets 'line_offsets', 'vp_offsets', 'out_offsets'."""
    if numClusters != 2:
        raise ValueError("numClusters = %r: only 2 is supported" % (numClusters,))
    lo = ragged.batch_offsets(linePoints, line_offsets, "linePoints")
    vo = ragged.batch_offsets(vs, vp_offsets, "vs")
    ragged.check_images(lo, vo, "linePoints", "vs")
    if ragged.total(weightMatrices) != ragged.mats_total(lo, vo):
        raise ValueError("the weight matrices do not hold the images' M x N elements")
    ragged.check_total(lines, lo[-1], "lines", 3, "rows")
    for x, n, what in ((ss, vo[-1], "ss"), (lineWeights, lo[-1], "lineWeights"), (lineAngles, lo[-1], "lineAngles")):
        ragged.check_total(x, n, what, unit="rows")
    B = lo.shape[0] - 1
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_lp = ragged.upload(rt, linePoints, np.float64, (4,))
        d_l = ragged.upload(rt, lines, np.float64, (3,))
        d_v = ragged.upload(rt, vs, np.float64, (3,))
        d_s = ragged.upload(rt, ss, np.float64)
        d_w = ragged.upload(rt, weightMatrices, np.float64)
        d_lw = ragged.upload(rt, lineWeights, np.float64)
        d_la = ragged.upload(rt, lineAngles, np.float64)
        oo = vo + np.arange(B + 1, dtype=np.int64)
        v_out = t.zeros((int(oo[-1]), 3), dtype=t.float64, device=rt.tdev)
        s_out = t.zeros((int(oo[-1]),), dtype=t.float64, device=rt.tdev)
        num = t.from_numpy(np.diff(vo).astype(np.int32)).to(rt.tdev)
        for b in np.nonzero((np.diff(lo) == 0) & (np.diff(vo) > 0))[0]:      # no lines: the set as it came
            v_out[int(oo[b]):int(oo[b]) + int(vo[b + 1] - vo[b])] = d_v[int(vo[b]):int(vo[b + 1])]
            s_out[int(oo[b]):int(oo[b]) + int(vo[b + 1] - vo[b])] = d_s[int(vo[b]):int(vo[b + 1])]
        split = t.full((B,), -1, dtype=t.int32, device=rt.tdev)
        flags = t.zeros((B,), dtype=t.int32, device=rt.tdev)
        labels = t.full((int(lo[-1]),), -1, dtype=t.int32, device=rt.tdev)
        rt.check(rt.lib.vpk_vp_split_batch(rt.h, B, ragged.off_ptr(lo), ragged.off_ptr(vo), rt.ptr(d_lp), rt.ptr(d_l), rt.ptr(d_v),
                                           rt.ptr(d_s), rt.ptr(d_w), rt.ptr(d_lw), rt.ptr(d_la), float(min_diff), rt.ptr(v_out),
                                           rt.ptr(s_out), rt.ptr(num), rt.ptr(split), rt.ptr(flags), rt.ptr(labels)))
    rt.synchronize()
    return {'v': v_out, 's': s_out, 'num_vp': num, 'split': split, 'flags': flags, 'labels': labels,
            'line_offsets': lo, 'vp_offsets': vo, 'out_offsets': oo}


def _history(v, s, i):
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 3 or v.shape[2] != 3:
        raise ValueError("v must be the (T, M, 3) history array (got shape %r)" % (v.shape,))
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    if s.shape[0] != v.shape[1]:
        raise ValueError("s holds %d variances for %d VPs" % (s.shape[0], v.shape[1]))
    if v.shape[1] > MAX_VP:
        raise ValueError("%d VPs: at most %d are supported" % (v.shape[1], MAX_VP))
    return v, s, v[i]


def split_best_vp(i, v, s, linePoints, lines, weightMatrix, lineWeights, lineAngles, numClusters=2, min_diff=0.0001, device=0):
    """split_best_vp (:527-630) on slice ``i`` of the (T, M, 3) history array ``v``: {'v', 's'}.  Where the worst VP is
    split, 'v' has one more VP: a zero column appended to every slice, and only slice i written (:626-628).  Returned
    arrays are new; the caller's v and s are not written."""
    if numClusters != 2:
        raise ValueError("numClusters = %r: only 2 is supported" % (numClusters,))
    v, s, vi = _history(v, s, i)
    M = v.shape[1]
    lp = _check_lp(linePoints)
    if M == 0 or lp.shape[0] == 0:
        return {'v': v.copy(), 's': s.copy()}
    r = split_best_vp_batch([vi], [s], [lp], [np.asarray(lines, dtype=np.float64)],
                            [np.asarray(weightMatrix, dtype=np.float64).reshape(M, -1)], [lineWeights], [lineAngles],
                            min_diff=min_diff, device=device)
    if int(r['split'][0]) < 0:
        return {'v': v.copy(), 's': s.copy()}
    v2 = np.append(v, np.zeros((v.shape[0], 1, 3)), axis=1)
    v2[i] = r['v'].cpu().numpy()[:M + 1]
    return {'v': v2, 's': r['s'].cpu().numpy()[:M + 1]}


def merge_vps_batch(vs, ss, ls, thresh, lweights, lsims, wbias, pdfpar, lps, llens=None, distance_measure="angle",
                    max_stdd=0.01, outlier_stdd=1e-6, line_offsets=None, vp_offsets=None, device=0):
    """merge_vps on slice i of many images' history arrays in one launch; arguments as in calc_vp_line_counts_batch (vs:
    (M_b, 3) each, ls (N_b, 3) normalised lines).  ``lsims``: the images' plain (N_b, N_b) matrices as a list -- the
    list calc_lsim_batch returns is used where it lies -- or concatenated flat.  ``pdfpar``: PDFParams with weights (B, 400),
    as pdf_params_batch returns.  ``llens`` is read by none of the reference's measures and is not used.
    ``distance_measure``: "angle", "dotprod" or "area", the measure of every round's E-step (:658); ``max_stdd`` is the
    caller's under each of them (the EM passes 0.01, :339, :448).  Returns a dict of device tensors: 'v'
    (sum M, 3), 's' (sum M,) and 'kept' (sum M,) int32: image b's rows start at vp_offsets[b], 'num_vp' (B,) of them are the
    merged set and the indices its VPs came with, the rest zeros and -1; 'flags' (B,) int32; and the host offsets.

    Everything may stay on the device:

        lscore, langle, llen, off = line_geometry_batch((d_lp, off), k1=10, k2=4)
        lsims = calc_lsim_batch((d_lp, off), sigma=1)
        par = pdf_params_batch(d_maps)
        r = merge_vps_batch(d_v, d_s, d_l, 1e-3, llen * lscore.clamp(0.2, 1), lsims, 1, par, d_lp,
                            line_offsets=off, vp_offsets=vp_off)"""
    measure = _measure_code(distance_measure)
    lo = ragged.batch_offsets(lps, line_offsets, "lps")
    vo = ragged.batch_offsets(vs, vp_offsets, "vs")
    ragged.check_images(lo, vo, "lps", "vs")
    B = lo.shape[0] - 1
    ragged.check_lsims(lsims, lo)
    if ragged.total(pdfpar.weights) != 400 * B:
        raise ValueError("pdfpar.weights must be (%d, 400), one row per image" % B)
    ragged.check_total(ls, lo[-1], "ls", 3, "rows")
    for x, n, what in ((ss, vo[-1], "ss"), (lweights, lo[-1], "lweights")):
        ragged.check_total(x, n, what, unit="rows")
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_lp = ragged.upload(rt, lps, np.float64, (4,))
        d_l = ragged.upload(rt, ls, np.float64, (3,))
        d_v = ragged.upload(rt, vs, np.float64, (3,))
        d_s = ragged.upload(rt, ss, np.float64)
        d_lw = ragged.upload(rt, lweights, np.float64)
        (lsim_ptr, lsim_keep), lsim_off = ragged.lsim_layout(rt, lsims, np.diff(lo))
        d_pw = ragged.upload(rt, pdfpar.weights, np.float32, (400,))
        v_out = d_v.clone()
        s_out = d_s.clone()
        num = t.from_numpy(np.diff(vo).astype(np.int32)).to(rt.tdev)
        kept = t.cat([t.arange(int(m), dtype=t.int32, device=rt.tdev) for m in np.diff(vo)]) if B else \
            t.zeros((0,), dtype=t.int32, device=rt.tdev)
        flags = t.zeros((B,), dtype=t.int32, device=rt.tdev)
        rt.check(rt.lib.vpk_vp_merge_batch_measure(rt.h, measure, B, ragged.off_ptr(lo), ragged.off_ptr(vo), rt.ptr(d_lp), rt.ptr(d_l),
                                                   rt.ptr(d_v), rt.ptr(d_s), rt.ptr(d_lw), ragged.off_ptr(lsim_off), lsim_ptr,
                                                   float(wbias), rt.ptr(d_pw), float(pdfpar.sigma), float(thresh), float(max_stdd),
                                                   rt.ptr(v_out), rt.ptr(s_out), rt.ptr(num), rt.ptr(kept), rt.ptr(flags)))
    rt.synchronize()
    del lsim_keep
    return {'v': v_out, 's': s_out, 'num_vp': num, 'kept': kept, 'flags': flags, 'line_offsets': lo, 'vp_offsets': vo}


def merge_vps(i, v, s, l, thresh, lweight, lsim, wbias, pdfpar, lp, llen, distance_measure, max_stdd=0.01, outlier_stdd=1e-6,
              device=0):
    """merge_vps (:633-684) on slice ``i`` of the (T, M, 3) history array ``v``: {'v', 's'}.  While the two closest VPs
    are closer than ``thresh``, they are merged into the second (column j is deleted from every slice, :674) until a merge
    is given up (new VP None, or s[k] > max_stdd -- s[k] is returned as changed, :666-668).  ``pdfpar`` is what this
    package's pdf_params returns.  Returned arrays are new; the caller's v and s are not written.
    This single-image form takes "angle" only; "dotprod" and "area": merge_vps_batch with one-image lists."""
    _check_measure(distance_measure)
    v, s, vi = _history(v, s, i)
    M = v.shape[1]
    lp = _check_lp(lp)
    if M <= 1 or lp.shape[0] == 0:
        return {'v': v.copy(), 's': s.copy()}
    if not np.array_equal(np.asarray(pdfpar.means), _grid_means()):
        raise ValueError("pdfpar.means must be the 20 x 20 grid of pdf_params")
    w = np.asarray(pdfpar.weights, dtype=np.float32).reshape(1, -1)
    if w.shape[1] != 400 or (w > 0).sum() > 100:
        raise ValueError("pdfpar.weights must be pdf_params' 400 cell weights, at most 100 of them positive")
    N = lp.shape[0]
    r = merge_vps_batch([vi], [s], [np.asarray(l, dtype=np.float64)], thresh, [lweight],
                        [np.asarray(lsim, dtype=np.float64).reshape(N, N)], wbias,
                        PDFParams(means=None, weights=w, sigma=pdfpar.sigma), [lp], max_stdd=max_stdd, device=device)
    m = int(r['num_vp'][0])
    kept = r['kept'].cpu().numpy()[:m]
    v2 = v[:, kept, :].copy()
    v2[i] = r['v'].cpu().numpy()[:m]
    return {'v': v2, 's': r['s'].cpu().numpy()[:m]}


# ---- the EM update outside the EM: weights, M-step and initial VPs for a batch ----------------------------------------------
MAX_LINES = ragged.MAX_LINES           # per image (csrc/vpk_emstep.hip)


def find_initial_vps_batch(sphere_images, cnn_responses, num_max, device=0, want_weights=False):
    """find_initial_vps for many images in one launch (vpk_init_vps_batch).  ``sphere_images``: (B, S, S) uint8, S >= 20,
    or a list of (S, S) images of one size; ``cnn_responses``: (B, 20, 20) float32 or a list.  Returns (v0 (B, num_max, 3)
    float64, num_vp (B,) int32) as device tensors: image b's VPs are v0[b, :num_vp[b]], the rows past them zeros, and
    num_vp[b] = 0 where the reference raises at :165.  ``want_weights``: a third tensor, the (B, 400) float32 pdf_params
    weights."""
    num_max = int(num_max)
    if num_max < 1 or num_max > MAX_VP:
        raise ValueError("num_max = %d: 1 to %d initial VPs are supported" % (num_max, MAX_VP))
    if ragged.is_list(sphere_images):
        sph = [ragged.shape(a) for a in sphere_images]
    else:
        if len(ragged.shape(sphere_images)) != 3:
            raise ValueError("sphere_images must be (B, S, S) or a list of (S, S) images")
        sph = [ragged.shape(sphere_images)[1:]] * ragged.shape(sphere_images)[0]
    B = len(sph)
    if any(len(s) != 2 or s[0] != s[1] or s != sph[0] for s in sph):
        raise ValueError("the sphere images must be square and of one size")
    if B and sph[0][0] < 20:
        raise ValueError("sphere images of %d pixels: at least 20 are needed" % sph[0][0])
    nc = len(cnn_responses) if ragged.is_list(cnn_responses) else (ragged.shape(cnn_responses)[0] if len(ragged.shape(cnn_responses)) else -1)
    if nc != B:
        raise ValueError("sphere_images and cnn_responses describe %d and %d images" % (B, nc))
    if ragged.is_list(cnn_responses):
        if any(ragged.numel(a) != 400 for a in cnn_responses):
            raise ValueError("every response map must hold 20 x 20 values")
    elif ragged.numel(cnn_responses) != 400 * B:
        raise ValueError("cnn_responses must hold 20 x 20 values per image")
    S = sph[0][0] if B else 20
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_cnn = ragged.upload(rt, cnn_responses, np.float32, (400,))
        d_sp = ragged.upload(rt, sphere_images, np.uint8, (S, S))
        v0 = t.zeros((B, num_max, 3), dtype=t.float64, device=rt.tdev)
        m0 = t.zeros((B,), dtype=t.int32, device=rt.tdev)
        wts = t.zeros((B, 400), dtype=t.float32, device=rt.tdev) if want_weights else None
        rt.check(rt.lib.vpk_init_vps_batch(rt.h, B, rt.ptr(d_cnn), rt.ptr(d_sp), S, num_max, rt.ptr(v0), rt.ptr(m0), rt.ptr(wts)))
    rt.synchronize()
    return (v0, m0, wts) if want_weights else (v0, m0)


def weight_matrix_batch(p_vls, lweights, lsims, bias=0.001, line_offsets=None, vp_offsets=None, device=0):
    """weight_matrix for many images in one launch (vpk_weight_matrix_batch).  ``p_vls``: a list of (M_b, N_b) arrays or
    tensors, or the matrices concatenated flat with ``line_offsets`` / ``vp_offsets``; ``lweights``: (N_b,) each or
    concatenated; ``lsims`` as in merge_vps_batch -- the list calc_lsim_batch returns is used where it lies.  ``bias``
    defaults to the reference's own 0.001; the EM calls weight_matrix with wbias (1).  Returns a list of (M_b, N_b) float64
    device tensors, views of one buffer in which the matrices follow each other without gaps."""
    lo = ragged.batch_offsets(lweights, line_offsets, "lweights")
    vo = ragged.vp_sizes_of_mats(p_vls, vp_offsets, "p_vls")
    ragged.check_counts(lo, vo, "lweights", "p_vls")
    ragged.check_mats(p_vls, lo, vo, "p_vls")
    ragged.check_lsims(lsims, lo)
    B = lo.shape[0] - 1
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_p = ragged.upload_mats(rt, p_vls)
        d_lw = ragged.upload(rt, lweights, np.float64)
        (lsim_ptr, lsim_keep), lsim_off = ragged.lsim_layout(rt, lsims, np.diff(lo))
        w = t.zeros((ragged.mats_total(lo, vo),), dtype=t.float64, device=rt.tdev)
        rt.check(rt.lib.vpk_weight_matrix_batch(rt.h, B, ragged.off_ptr(lo), ragged.off_ptr(vo), rt.ptr(d_p), rt.ptr(d_lw),
                                                ragged.off_ptr(lsim_off), lsim_ptr, float(bias), rt.ptr(w)))
    rt.synchronize()
    del lsim_keep
    return ragged.split_mats(w, lo, vo)


def calc_new_vanishing_point_batch(ls, ws, line_offsets=None, vp_offsets=None, device=0):
    """calc_new_vanishing_point for every row of many images' weight matrices in one launch (vpk_mstep_batch without
    state).  ``ls``: (N_b, 3) normalised lines each, ``ws``: (M_b, N_b) each -- or concatenated with the offsets.  Returns
    (vp (sum M, 3) float64, valid (sum M,) int32) as device tensors: vp is zero and valid 0 where the reference returns None."""
    lo = ragged.batch_offsets(ls, line_offsets, "ls")
    vo = ragged.vp_sizes_of_mats(ws, vp_offsets, "ws")
    ragged.check_counts(lo, vo, "ls", "ws")
    ragged.check_rows(ls, lo, 3, "ls")
    ragged.check_mats(ws, lo, vo, "ws")
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_l = ragged.upload(rt, ls, np.float64, (3,))
        d_w = ragged.upload_mats(rt, ws)
        vp = t.zeros((int(vo[-1]), 3), dtype=t.float64, device=rt.tdev)
        valid = t.zeros((int(vo[-1]),), dtype=t.int32, device=rt.tdev)
        rt.check(rt.lib.vpk_mstep_batch(rt.h, lo.shape[0] - 1, ragged.off_ptr(lo), ragged.off_ptr(vo), rt.ptr(d_l), rt.ptr(d_w), None, None,
                                        None, None, 1e-6, 1e-200, rt.ptr(vp), None, None, None, rt.ptr(valid), None))
    rt.synchronize()
    return vp, valid


def mstep_batch(ls, ws, lvsqs, p_vls, curs, assocs=None, max_stdd=1e-6, s_thresh=1e-200, line_offsets=None, vp_offsets=None,
                device=0):
    """The M-step of one EM iteration (:284-322; with ``assocs`` the hard one, :353-392) for many images in one launch
    (vpk_mstep_batch).  Per image: ``ls`` (N_b, 3) normalised lines, ``ws`` (M_b, N_b) the decision metric, ``lvsqs``
    (N_b, M_b) and ``p_vls`` (M_b, N_b) -- the shapes of the reference's PDF.lvsq and PDF.vl, so the tuples of
    calc_probabilities_batch pass on unchanged --, ``curs`` (M_b, 3) the VPs of the previous iteration, ``assocs`` (N_b,)
    int64 as calc_vp_line_counts_batch returns it (-1 selects no VP).  Lists, or concatenated with ``line_offsets`` /
    ``vp_offsets`` (matrices then flat as [m][n], image after image).  Returns a dict of device tensors: 'v' (sum M, 3), 's'
    and 'err' (sum M,), 'removed' and 'valid' (sum M,) int32, 'max_err' (B,) -- rows the M-step does not write are v = 0,
    s = -1, err = -1; max_err of an image without lines or VPs is 0 -- and the host 'line_offsets', 'vp_offsets'.

    One iteration that stays on the device (lps, ls: lists of per-image device tensors; off: the host offsets):

        pair = (torch.cat(lps), off)
        lsims = calc_lsim_batch(pair, sigma=1)
        lscore, langle, llen, off = line_geometry_batch(pair, k1=10, k2=4)
        lw = llen * lscore.clamp(0.2, 1)
        v0, num = find_initial_vps_batch(spheres, maps, 25)
        vs = [v0[b, :k] for b, k in enumerate(num.tolist())]              # (B counts: the one host copy)
        e = calc_probabilities_batch(maps, vs, ls, lps, [v.new_full((len(v),), 1.2e-7) for v in vs])
        w = weight_matrix_batch([p.vl for p in e['pdf']], lw, lsims, bias=1, line_offsets=off)
        r = mstep_batch(ls, w, [p.lvsq for p in e['pdf']], [p.vl for p in e['pdf']], vs)
        counts, counts_w, assoc, _, _ = calc_vp_line_counts_batch(r['v'], pair[0], r['s'], w, lw, line_offsets=off,
                                                                  vp_offsets=r['vp_offsets'])"""
    if (lvsqs is None) != (p_vls is None):
        raise ValueError("lvsqs and p_vls are given together (calc_new_vanishing_point_batch takes neither)")
    if lvsqs is None:
        raise ValueError("mstep_batch needs lvsqs and p_vls: calc_new_vanishing_point_batch gives the positions alone")
    lo = ragged.batch_offsets(ls, line_offsets, "ls")
    vo = ragged.batch_offsets(curs, vp_offsets, "curs")
    ragged.check_counts(lo, vo, "ls", "curs")
    ragged.check_rows(ls, lo, 3, "ls")
    ragged.check_rows(curs, vo, 3, "curs")
    ragged.check_mats(ws, lo, vo, "ws")
    ragged.check_mats(lvsqs, lo, vo, "lvsqs", transposed=True)
    ragged.check_mats(p_vls, lo, vo, "p_vls")
    if assocs is not None:
        ragged.check_rows(assocs, lo, 1, "assocs")
    B = lo.shape[0] - 1
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_l = ragged.upload(rt, ls, np.float64, (3,))
        d_cur = ragged.upload(rt, curs, np.float64, (3,))
        d_w, d_lv, d_p = ragged.upload_mats(rt, ws), ragged.upload_mats(rt, lvsqs, transposed=True), ragged.upload_mats(rt, p_vls)
        d_a = ragged.upload(rt, assocs, np.int64) if assocs is not None else None
        M = int(vo[-1])
        vp = t.zeros((M, 3), dtype=t.float64, device=rt.tdev)
        s = t.full((M,), -1.0, dtype=t.float64, device=rt.tdev)
        err = t.full((M,), -1.0, dtype=t.float64, device=rt.tdev)
        removed = t.zeros((M,), dtype=t.int32, device=rt.tdev)
        valid = t.zeros((M,), dtype=t.int32, device=rt.tdev)
        max_err = t.zeros((B,), dtype=t.float64, device=rt.tdev)
        rt.check(rt.lib.vpk_mstep_batch(rt.h, B, ragged.off_ptr(lo), ragged.off_ptr(vo), rt.ptr(d_l), rt.ptr(d_w), rt.ptr(d_lv), rt.ptr(d_p),
                                        rt.ptr(d_a), rt.ptr(d_cur), float(max_stdd), float(s_thresh), rt.ptr(vp), rt.ptr(s),
                                        rt.ptr(err), rt.ptr(removed), rt.ptr(valid), rt.ptr(max_err)))
    rt.synchronize()
    return {'v': vp, 's': s, 'err': err, 'removed': removed, 'valid': valid, 'max_err': max_err, 'line_offsets': lo,
            'vp_offsets': vo}


def calc_angle_to_other_vp(v, i, k):
    """calc_angle_to_other_vp (:687-697), on the host: the angles of VP k of slice i against every VP of the slice, pi
    for itself -- and the scalar pi where squeezing leaves a single VP (:693-694)."""
    vi = np.asarray(v)[i]
    d = np.dot(np.squeeze(vi), np.squeeze(vi[k]).T)
    ang = np.abs(np.arccos(np.clip(np.abs(np.clip(d, -1, 1)), -1, 1)))
    if np.ndim(ang) == 0:
        return np.pi
    ang[k] = np.pi
    return ang
