"""Host-in / host-out wrappers of the fine-grained C-ABI entry points (unit parity against the
reference's individual functions).  Each call copies its inputs to HBM, launches one workgroup
and copies the result back -- for tests and debugging, not for throughput."""
import numpy as np

from .ragged import to_device as _up
from .runtime import get_runtime


def pairwise(lp, device=0):
    """calc_lsim (vp_localisation.py:87-108) + line_rating_knn (:34-84) + lines_angles (:765-776)."""
    rt = get_runtime(device)
    t = rt.torch
    n = lp.shape[0]
    with rt.on_stream():
        d_lp = _up(rt, lp, np.float64)
        lsim = t.empty((n, n), dtype=t.float64, device=rt.tdev)
        lscore = t.empty((n,), dtype=t.float64, device=rt.tdev)
        langle = t.empty((n,), dtype=t.float64, device=rt.tdev)
        rt.check(rt.lib.vpk_pairwise(rt.h, n, rt.ptr(d_lp), rt.ptr(lsim), rt.ptr(lscore), rt.ptr(langle)))
    rt.synchronize()
    return lsim.cpu().numpy(), lscore.cpu().numpy(), langle.cpu().numpy()


def init_vps(cnn, sphere, num_max=25, device=0):
    """find_initial_vps (vp_localisation.py:111-165) + pdf_params weights (probability_functions.py:62-96)."""
    rt = get_runtime(device)
    t = rt.torch
    with rt.on_stream():
        d_cnn = _up(rt, np.asarray(cnn).reshape(400), np.float32)
        d_sp = _up(rt, sphere, np.uint8)
        v0 = t.zeros((64, 3), dtype=t.float64, device=rt.tdev)
        m0 = t.zeros((1,), dtype=t.int32, device=rt.tdev)
        w = t.zeros((400,), dtype=t.float32, device=rt.tdev)
        rt.check(rt.lib.vpk_init_vps(rt.h, rt.ptr(d_cnn), rt.ptr(d_sp), int(sphere.shape[0]), int(num_max),
                                     rt.ptr(v0), rt.ptr(m0), rt.ptr(w)))
    rt.synchronize()
    m = int(m0.cpu()[0])
    return v0.cpu().numpy()[:m], w.cpu().numpy()


def estep(lp, cnn, v, s, device=0):
    """calc_probabilities (probability_functions.py:99-120). Returns p_v, lvsq (N,M), p_vl (M,N), p_l, s."""
    rt = get_runtime(device)
    t = rt.torch
    n, m = lp.shape[0], v.shape[0]
    with rt.on_stream():
        d_lp = _up(rt, lp, np.float64)
        d_cnn = _up(rt, np.asarray(cnn).reshape(400), np.float32)
        d_v = _up(rt, v, np.float64)
        d_s = _up(rt, s, np.float64)
        pv = t.empty((m,), dtype=t.float64, device=rt.tdev)
        lvsq = t.empty((m, n), dtype=t.float64, device=rt.tdev)
        pvl = t.empty((m, n), dtype=t.float64, device=rt.tdev)
        pl = t.empty((n,), dtype=t.float64, device=rt.tdev)
        rt.check(rt.lib.vpk_estep(rt.h, n, m, rt.ptr(d_lp), rt.ptr(d_cnn), rt.ptr(d_v), rt.ptr(d_s), rt.ptr(pv),
                                  rt.ptr(lvsq), rt.ptr(pvl), rt.ptr(pl)))
    rt.synchronize()
    return pv.cpu().numpy(), lvsq.cpu().numpy().T.copy(), pvl.cpu().numpy(), pl.cpu().numpy(), d_s.cpu().numpy()


def weight_matrix(p_vl, lweight, lsim, bias=1.0, device=0):
    """weight_matrix (vp_localisation.py:515-524)."""
    rt = get_runtime(device)
    t = rt.torch
    m, n = p_vl.shape
    with rt.on_stream():
        d_p = _up(rt, p_vl, np.float64)
        d_lw = _up(rt, lweight, np.float64)
        d_ls = _up(rt, lsim, np.float64)
        w = t.empty((m, n), dtype=t.float64, device=rt.tdev)
        rt.check(rt.lib.vpk_weight_matrix(rt.h, n, m, rt.ptr(d_p), rt.ptr(d_lw), rt.ptr(d_ls), float(bias), rt.ptr(w)))
    rt.synchronize()
    return w.cpu().numpy()


def estep_smooth(lp, cnn, v, s, lweight, lsim, bias=1.0, device=0):
    """calc_probabilities followed by weight_matrix in one workgroup, the smoother taking the operand panel the E-step left
    in LDS where it planned one (vpk_estep_smooth, a test hook).  Returns p_vl (M,N), w (M,N), s (floored), info (4 int32)."""
    rt = get_runtime(device)
    t = rt.torch
    n, m = lp.shape[0], v.shape[0]
    with rt.on_stream():
        d_lp, d_v, d_s = _up(rt, lp, np.float64), _up(rt, v, np.float64), _up(rt, s, np.float64)
        d_cnn = _up(rt, np.asarray(cnn).reshape(400), np.float32)
        d_lw, d_ls = _up(rt, lweight, np.float64), _up(rt, lsim, np.float64)
        pvl = t.empty((m, n), dtype=t.float64, device=rt.tdev)
        w = t.empty((m, n), dtype=t.float64, device=rt.tdev)
        info = t.zeros((4,), dtype=t.int32, device=rt.tdev)
        rt.check(rt.lib.vpk_estep_smooth(rt.h, n, m, rt.ptr(d_lp), rt.ptr(d_cnn), rt.ptr(d_v), rt.ptr(d_s), rt.ptr(d_lw),
                                         rt.ptr(d_ls), float(bias), rt.ptr(pvl), rt.ptr(w), rt.ptr(info)))
    rt.synchronize()
    return pvl.cpu().numpy(), w.cpu().numpy(), d_s.cpu().numpy(), info.cpu().numpy()


def mstep(l, w, device=0):
    """calc_new_vanishing_point (vp_localisation.py:453-479) for every row of w (M,N)."""
    rt = get_runtime(device)
    t = rt.torch
    m, n = w.shape
    with rt.on_stream():
        d_l = _up(rt, l, np.float64)
        d_w = _up(rt, w, np.float64)
        vp = t.empty((m, 3), dtype=t.float64, device=rt.tdev)
        valid = t.empty((m,), dtype=t.int32, device=rt.tdev)
        rt.check(rt.lib.vpk_mstep(rt.h, n, m, rt.ptr(d_l), rt.ptr(d_w), rt.ptr(vp), rt.ptr(valid)))
    rt.synchronize()
    return vp.cpu().numpy(), valid.cpu().numpy()


def mstep_full(l, w, lvsq, p_vl, cur, assoc=None, max_stdd=1e-6, s_thresh=1e-200, device=0):
    """The whole M-step of one iteration (vp_localisation.py:284-322; with ``assoc`` the hard one, :353-392) on supplied
    state: w, lvsq, p_vl (M,N), cur (M,3).  Returns vp (M,3), s, err, removed (vpk_mstep_full, a test hook)."""
    rt = get_runtime(device)
    t = rt.torch
    m, n = w.shape
    with rt.on_stream():
        d_l, d_w = _up(rt, l, np.float64), _up(rt, w, np.float64)
        d_lv, d_p, d_cur = _up(rt, lvsq, np.float64), _up(rt, p_vl, np.float64), _up(rt, cur, np.float64)
        d_a = None if assoc is None else _up(rt, assoc, np.int32)
        vp = t.empty((m, 3), dtype=t.float64, device=rt.tdev)
        s = t.empty((m,), dtype=t.float64, device=rt.tdev)
        err = t.empty((m,), dtype=t.float64, device=rt.tdev)
        removed = t.empty((m,), dtype=t.int32, device=rt.tdev)
        rt.check(rt.lib.vpk_mstep_full(rt.h, n, m, rt.ptr(d_l), rt.ptr(d_w), rt.ptr(d_lv), rt.ptr(d_p),
                                       None if d_a is None else rt.ptr(d_a), rt.ptr(d_cur), float(max_stdd), float(s_thresh),
                                       rt.ptr(vp), rt.ptr(s), rt.ptr(err), rt.ptr(removed)))
    rt.synchronize()
    return vp.cpu().numpy(), s.cpu().numpy(), err.cpu().numpy(), removed.cpu().numpy()


def line_counts(lp, v, s, w, lweight, thresh=1.96 ** 2, device=0):
    """calc_vp_line_counts (vp_localisation.py:482-512): returns (counts, counts_weighted, assoc)."""
    rt = get_runtime(device)
    t = rt.torch
    m, n = w.shape
    with rt.on_stream():
        d_lp, d_v, d_s = _up(rt, lp, np.float64), _up(rt, v, np.float64), _up(rt, s, np.float64)
        d_w, d_lw = _up(rt, w, np.float64), _up(rt, lweight, np.float64)
        counts = t.empty((m,), dtype=t.float64, device=rt.tdev)
        counts_w = t.empty((m,), dtype=t.float64, device=rt.tdev)
        assoc = t.empty((n,), dtype=t.int64, device=rt.tdev)
        rt.check(rt.lib.vpk_line_counts(rt.h, n, m, rt.ptr(d_lp), rt.ptr(d_v), rt.ptr(d_s), rt.ptr(d_w), rt.ptr(d_lw),
                                        float(thresh), rt.ptr(counts), rt.ptr(counts_w), rt.ptr(assoc)))
    rt.synchronize()
    return counts.cpu().numpy(), counts_w.cpu().numpy(), assoc.cpu().numpy()


def cluster2(ldist, device=0):
    """The 2-cluster average-linkage agglomeration of split_best_vp (vp_localisation.py:568-578)."""
    rt = get_runtime(device)
    t = rt.torch
    n = ldist.shape[0]
    with rt.on_stream():
        d = _up(rt, ldist, np.float64)
        labels = t.empty((n,), dtype=t.int32, device=rt.tdev)
        flags = t.zeros((1,), dtype=t.int32, device=rt.tdev)
        rt.check(rt.lib.vpk_cluster2(rt.h, n, rt.ptr(d), rt.ptr(labels), rt.ptr(flags)))
    rt.synchronize()
    return labels.cpu().numpy(), int(flags.cpu()[0])


def build_records(image_ids, vp, counts, num_vp, status, max_vp, device=0):
    """vpk_build_records (include/vpk.h): the fixed-size result records of a batch, (B, vpk_record_width()) float64.
    image_ids B int64, vp B x max_vp x 3, counts B x max_vp, num_vp and status B int32."""
    rt = get_runtime(device)
    t = rt.torch
    batch = int(np.asarray(image_ids).shape[0])
    vp, counts = np.asarray(vp, dtype=np.float64), np.asarray(counts, dtype=np.float64)
    if vp.shape != (batch, max_vp, 3) or counts.shape != (batch, max_vp) or len(num_vp) != batch or len(status) != batch:
        raise ValueError("build_records: vp must be B x max_vp x 3, counts B x max_vp, num_vp and status B")
    with rt.on_stream():
        d_id, d_vp, d_cnt = _up(rt, image_ids, np.int64), _up(rt, vp, np.float64), _up(rt, counts, np.float64)
        d_num, d_st = _up(rt, num_vp, np.int32), _up(rt, status, np.int32)
        rec = t.empty((batch, int(rt.lib.vpk_record_width())), dtype=t.float64, device=rt.tdev)
        rt.check(rt.lib.vpk_build_records(rt.h, batch, int(max_vp), rt.ptr(d_id), rt.ptr(d_vp), rt.ptr(d_cnt), rt.ptr(d_num),
                                          rt.ptr(d_st), rt.ptr(rec)))
    rt.synchronize()
    return rec.cpu().numpy()


MATH_FUNCTIONS = ("exp", "acos", "asin", "atan", "sqrt", "sin", "cos", "log")


def math_probe(name, x, device=0):
    """The device's double-precision elementary function ``name`` (as the EM kernels call it) on every element of x."""
    rt = get_runtime(device)
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    dx = _up(rt, x, np.float64)
    with rt.on_stream():
        dy = rt.torch.empty_like(dx)
        rt.check(rt.lib.vpk_math_probe(rt.h, MATH_FUNCTIONS.index(name), int(x.shape[0]), rt.ptr(dx), rt.ptr(dy)))
    rt.synchronize()
    return dy.cpu().numpy()
