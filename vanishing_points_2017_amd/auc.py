"""Horizon-error AUC -- port of the reference's auc.calc_auc (auc.py:5-37): sorted errors ->
cumulative fraction curve, value at the cutoff interpolated as at :20-28, trapezoid area / cutoff."""
import numpy as np

_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def calc_auc(error_array, cutoff=0.25):
    err = np.sort(np.asarray(error_array).squeeze())
    n = err.shape[0]
    pts = np.zeros((n, 2))
    pts[:, 0] = err
    pts[:, 1] = (np.arange(n) + 1) * 1.0 / n
    mid = 1.
    for i in range(1, n):                         # the last crossing wins, as in the reference loop
        if err[i - 1] < cutoff < err[i]:
            mid = (err[i - 1] * pts[i - 1, 1] + err[i] * pts[i, 1]) / (err[i] + err[i - 1])
    tail = np.array([cutoff, 1]) if pts[-1, 0] < cutoff else np.array([cutoff, mid])
    pts = np.vstack([pts, tail])
    pts = pts[np.argsort(pts[:, 0]), :]
    sel = pts[:, 0] <= cutoff
    auc = _trapezoid(pts[sel, 1], pts[sel, 0])    # sklearn.metrics.auc == trapezoid rule (auc.py:33)
    return auc / cutoff, pts


def calc_auc_device(rt, err, cutoff=0.25):
    """calc_auc on a device vector of errors (vpk_auc): returns (auc, sorted_errors) -- the AUC as a Python float, the
    errors in np.sort's order (NaN last) as a device tensor.  Ties follow np.argsort(kind="stable") (include/vpk.h).
    1 <= n <= 65536.  The call waits for the stream only to hand back the one number."""
    torch = rt.torch
    if err.dtype != torch.float64 or err.dim() != 1:
        raise ValueError("calc_auc_device expects a one-dimensional float64 device tensor")
    n = int(err.shape[0])
    with rt.on_stream():
        err = err.contiguous()
        srt = torch.empty((max(n, 1),), dtype=torch.float64, device=rt.tdev)[:n]
        out = torch.empty((1,), dtype=torch.float64, device=rt.tdev)
        rt.check(rt.lib.vpk_auc(rt.h, n, rt.ptr(err), float(cutoff), rt.ptr(srt), rt.ptr(out)))
        auc = float(out.cpu()[0])
    return auc, srt
