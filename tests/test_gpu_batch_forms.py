"""Every ``*_batch`` function of vp_localisation and probability_functions through every form of input it accepts -- a list of
NumPy arrays, a list of device tensors, concatenated (on the host or on the device) with offsets, the (device tensor,
offsets) pair of the line functions -- on one batch of three images with 5, 0 and 3 lines and 2, 1 and 0 VPs: the smallest
in which a wrong offset, a wrong stride or a missed empty image shows.  The forms must give the same bits and leave the
caller's data as it was.  What the values are held to is the business of each function's own tests."""
import numpy as np
import pytest

import estep_reference as R

pytestmark = pytest.mark.gpu

N, M = (5, 0, 3), (2, 1, 0)
LO, VO = np.array([0, 5, 5, 8], np.int64), np.array([0, 2, 3, 3], np.int64)


def _torch():
    import torch
    return torch


def dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def same(a, b):
    """bit for bit, so NaNs compare as equal; lists, tuples, dicts and the host offsets element by element"""
    torch = _torch()
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    if not isinstance(a, torch.Tensor):
        return a == b
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


@pytest.fixture(scope="module")
def batch():
    """The images as host arrays, key by key one list entry per image; generated once and never changed."""
    rs = np.random.RandomState(11)
    ims = [R.case(n, m) for n, m in zip(N, M)]
    out = {k: [im[k] for im in ims] for k in ("lp", "l", "v", "s")}
    out["w"] = [rs.rand(m, n) for n, m in zip(N, M)]
    out["p_vl"] = [rs.rand(m, n) for n, m in zip(N, M)]
    out["lvsq"] = [rs.rand(n, m) * 1e-3 for n, m in zip(N, M)]                       # (N, M), as PDF.lvsq
    out["lw"] = [rs.uniform(0.2, 1.0, n) for n in N]
    out["assoc"] = [rs.randint(-1, max(m, 1), n).astype(np.int64) for n, m in zip(N, M)]
    out["maps"] = (rs.rand(3, 20, 20) ** 4).astype(np.float32)
    return out


class Forms(object):
    """The forms of one batch, and the check that a call left every one of them as it was."""

    def __init__(self, batch):
        self.host = dict(batch)
        self.dev = {k: [dev(a) for a in v] for k, v in batch.items() if k != "maps"}
        self.cat = {k: np.concatenate([a.ravel() if k in ("w", "p_vl", "s", "lw", "assoc") else a for a in v])
                    for k, v in batch.items() if k not in ("maps", "lvsq")}
        self.cat["lvsq"] = np.concatenate([a.T.ravel() for a in batch["lvsq"]])          # flat matrices are [m][n]
        self.dcat = {k: dev(a) for k, a in self.cat.items()}
        self.kept = self.snapshot()

    def add(self, key, arrays):
        """a further input made on the way (line angles, similarity matrices): host arrays in, all four forms kept"""
        self.host[key] = [np.array(a) for a in arrays]
        self.dev[key] = [dev(a) for a in arrays]
        self.cat[key] = np.concatenate([a.ravel() for a in self.host[key]])
        self.dcat[key] = dev(self.cat[key])
        self.kept = self.snapshot()

    def snapshot(self):
        return ({k: [np.array(a) for a in v] for k, v in self.host.items() if k != "maps"},
                {k: [a.clone() for a in v] for k, v in self.dev.items()},
                {k: a.copy() for k, a in self.cat.items()}, {k: a.clone() for k, a in self.dcat.items()})

    def untouched(self):
        h, d, c, dc = self.kept
        return all(same(self.host[k], h[k]) for k in h) and same(self.dev, d) and same(self.cat, c) and same(self.dcat, dc)

    def lists(self, *keys):
        """(form name, arguments) for the two list forms"""
        return [("numpy list", [self.host[k] for k in keys]), ("tensor list", [self.dev[k] for k in keys])]

    def all(self, *keys):
        """... and for the two concatenated forms, which go with line_offsets / vp_offsets"""
        return self.lists(*keys) + [("numpy concatenated", [self.cat[k] for k in keys]), ("tensor concatenated", [self.dcat[k] for k in keys])]


def agree(forms, results):
    first = results[0]
    for name, r in results[1:]:
        assert same(first[1], r), "%s differs from %s" % (name, first[0])
    assert forms.untouched(), "a caller's array or tensor was written"
    return first[1]


def off(name):
    return {"line_offsets": LO, "vp_offsets": VO} if "concatenated" in name else {}


def test_every_input_form_gives_the_same_bits(batch):
    from vanishing_points_2017_amd import probability_functions as P, vp_localisation as V
    torch = _torch()
    f = Forms(batch)
    maps, d_maps = batch["maps"], dev(batch["maps"])
    pair = (f.dcat["lp"], LO)

    # line geometry: a list of arrays, or the pair; k1 = 2, k2 = 1: the image of three lines has two neighbours per line
    lsims = agree(f, [("numpy list", V.calc_lsim_batch(f.host["lp"], sigma=1)), ("pair", V.calc_lsim_batch(pair, sigma=1))])
    assert [tuple(a.shape) for a in lsims] == [(n, n) for n in N]
    geo = agree(f, [("numpy list", V.line_geometry_batch(f.host["lp"], k1=2, k2=1)), ("pair", V.line_geometry_batch(pair, k1=2, k2=1))])
    lscore, langle, llen, lo = geo
    assert np.array_equal(lo, LO) and all(tuple(a.shape) == (8,) for a in (lscore, langle, llen))
    f.add("langle", [langle[LO[b]:LO[b + 1]].cpu().numpy() for b in range(3)])
    f.add("lsim", [a.cpu().numpy() for a in lsims])

    # the E-step: lists of arrays or of tensors
    for measure in ("angle", "dotprod", "area"):
        lv = agree(f, [(name, P.calc_lvsq_batch(*a, distance_measure=measure)) for name, a in f.lists("v", "l", "lp")])
        assert [tuple(a.shape) for a in lv] == list(zip(N, M))
        for prior in (maps, d_maps):
            e = agree(f, [(name, P.calc_probabilities_batch(prior, *a, distance_measure=measure)) for name, a in f.lists("v", "l", "lp", "s")])
        assert same(e["pdf"][0].lvsq, lv[0]) and tuple(e["pdf"][0].vl.shape) == (2, 5) and tuple(e["pdf"][2].lv.shape) == (3, 0)
        assert np.array_equal(e["line_offsets"], LO) and np.array_equal(e["vp_offsets"], VO)

    # the EM update: every form; the similarity matrices also as calc_lsim_batch's own views, which are used where they lie
    res = [(name, V.weight_matrix_batch(p, lw, ls, bias=1, **off(name))) for name, (p, lw, ls) in f.all("p_vl", "lw", "lsim")]
    res.append(("views", V.weight_matrix_batch(f.dev["p_vl"], f.dev["lw"], lsims, bias=1)))
    w = agree(f, res)
    assert [tuple(a.shape) for a in w] == list(zip(M, N))
    vp, valid = agree(f, [(name, V.calc_new_vanishing_point_batch(*a, **off(name))) for name, a in f.all("l", "w")])
    assert tuple(vp.shape) == (3, 3) and tuple(valid.shape) == (3,)
    for hard in (False, True):
        res = [(name, V.mstep_batch(*a[:5], assocs=a[5] if hard else None, **off(name)))
               for name, a in f.all("l", "w", "lvsq", "p_vl", "v", "assoc")]
        r = agree(f, res)
        assert tuple(r["v"].shape) == (3, 3) and tuple(r["max_err"].shape) == (3,) and float(r["max_err"][1]) == 0.0

    # VP set maintenance: every form
    for assoc in (False, True):
        res = [(name, V.calc_vp_line_counts_batch(v, lp, s, None if assoc else w, lw, vp_assocs=a if assoc else None, **off(name)))
               for name, (v, lp, s, w, lw, a) in f.all("v", "lp", "s", "w", "lw", "assoc")]
        counts, counts_w, a_out, lo, vo = agree(f, res)
        assert tuple(counts.shape) == (3,) and tuple(a_out.shape) == (8,) and np.array_equal(lo, LO) and np.array_equal(vo, VO)
    r = agree(f, [(name, V.split_best_vp_batch(*a, **off(name))) for name, a in f.all("v", "s", "lp", "l", "w", "lw", "langle")])
    assert tuple(r["v"].shape) == (6, 3) and r["out_offsets"].tolist() == [0, 3, 5, 6] and r["num_vp"].tolist()[1:] == [1, 0]
    par = P.pdf_params_batch(d_maps)
    res = []
    for weights in (par.weights, par.weights.cpu().numpy()):
        pp = P.PDFParams(means=None, weights=weights, sigma=par.sigma)
        res += [(name + (", host prior" if weights is not par.weights else ""),
                 V.merge_vps_batch(v, s, l, 1e-3, lw, ls, 1, pp, lp, **off(name)))
                for name, (v, s, l, lw, ls, lp) in f.all("v", "s", "l", "lw", "lsim", "lp")]
    res.append(("views", V.merge_vps_batch(f.dev["v"], f.dev["s"], f.dev["l"], 1e-3, f.dev["lw"], lsims, 1, par, f.dev["lp"])))
    r = agree(f, res)
    assert tuple(r["v"].shape) == (3, 3) and r["num_vp"].tolist()[1:] == [1, 0]
    torch.cuda.synchronize()
