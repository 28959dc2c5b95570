"""Batches for the batched EM update (csrc/emstep_device.hpp), shared by tests/test_emstep.py (the host build) and
tests/test_gpu_emstep.py (the kernel).  The images are the cases of tests/em_smoother_reference.py and
tests/em_phase_reference.py, imported as they are; what is new here is only how they are put into one ragged batch:
out of size order (the launch order is largest first, so input order and launch order differ) and interleaved with images
that have no lines or no VPs."""
import functools
import os

import numpy as np

import em_phase_reference as R
import em_smoother_reference as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emstep")
EMPTY = [(0, 3), (5, 0), (0, 0)]        # (N, M) of images that get no work


def interleave(images, make_empty):
    """The images with an empty one (N = 0 or M = 0, in turn) before every third of them and one at the end."""
    out = []
    for i, im in enumerate(images):
        if i % 3 == 0:
            out.append(make_empty(*EMPTY[(i // 3) % 3]))
        out.append(im)
    out.append(make_empty(*EMPTY[1]))
    return out


def offsets(images, key_n, key_m):
    lo = np.concatenate(([0], np.cumsum([im[key_n].shape[0] for im in images]))).astype(np.int64)
    vo = np.concatenate(([0], np.cumsum([im[key_m].shape[0] for im in images]))).astype(np.int64)
    return lo, vo


# ---- weights --------------------------------------------------------------------------------------------------------------
def _empty_weights(n, m):
    return {"p_vl": np.zeros((m, n)), "lweight": np.zeros(n), "lsim": np.zeros((n, n)), "n": n, "m": m}


@functools.lru_cache(maxsize=None)
def weight_images(shapes):
    """sparse_case of every shape, interleaved with empty images; ``shapes`` a tuple of (N, M)."""
    ims = []
    for n, m in shapes:
        c = dict(S.sparse_case(n, m))
        c.update(n=n, m=m)
        ims.append(c)
    return interleave(ims, _empty_weights)


@functools.lru_cache(maxsize=None)
def weight_reference(shapes, bias):
    """Per image with work: (extended reference, bar) of smooth_reference with exact operands (b_w = 0)."""
    return [S.smooth_reference(im["p_vl"] * im["lweight"][None, :], 0 * im["p_vl"], im["lweight"], im["lsim"], bias)
            if im["n"] and im["m"] else None for im in weight_images(shapes)]


# ---- M-step ---------------------------------------------------------------------------------------------------------------
def _empty_mstep(n, m):
    return {"l": np.zeros((n, 3)), "w": np.zeros((m, n)), "lvsq": np.zeros((m, n)), "p_vl": np.zeros((m, n)),
            "assoc": np.zeros(n, dtype=np.int64), "cur": np.zeros((m, 3)), "ref": None, "n": n, "m": m}


@functools.lru_cache(maxsize=None)
def mstep_images(shapes, hard):
    """mstep_case of every shape with its extended reference and previous VPs (mstep_cur), interleaved with empty images.
    Hard mode: the association as int64; where a case leaves a VP without lines by pointing them at VP (k + 1) % M the
    first such line is pointed at -1 and the second at M + 7 instead -- entries outside [0, M), which select no VP."""
    ims = []
    for n, m in shapes:
        c = dict(R.mstep_case(n, m, hard))
        if hard:
            a = c["assoc"].astype(np.int64)
            moved = np.nonzero(a != np.arange(n) % m)[0]
            for j, q in enumerate(moved[:2]):
                others = np.nonzero(a == a[q])[0]
                if others.size > 1:                          # (never the last line of a VP: its kind would change)
                    a[q] = -1 if j == 0 else m + 7
            c["assoc"] = a
            c["assoc32"] = np.where((a < 0) | (a >= m), -1, a).astype(np.int32)
        ref = R.mstep_reference(c["l"], c["w"], c["lvsq"], c["p_vl"], None, c.get("assoc32") if hard else None,
                                R.MSTEP_MAX_STDD, R.MSTEP_S_THRESH)
        c["ref"] = ref
        c["cur"] = R.mstep_cur(c, ref, lambda k: k % 12)
        c.update(n=n, m=m)
        ims.append(c)
    return interleave(ims, _empty_mstep)


def max_err_reference(err):
    """max_err_of: the np.maximum chain from 0 over the errors that are not -1; a NaN sticks."""
    mx = 0.0
    for e in err:
        if e != -1.0:
            mx = np.maximum(mx, e)
    return mx


# ---- goldens --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def golden_cases(name, suffix):
    return sorted(k[:-len(suffix)] for k in golden(name) if k.endswith(suffix))
