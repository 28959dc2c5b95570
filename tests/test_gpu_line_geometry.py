"""vpk_line_similarity_batch and vpk_line_rating_batch (csrc/vpk_lines.hip) and the vp_localisation call surface on top of
them, against the references and bars of tests/line_geometry_reference.py.

Shapes: a similarity workgroup takes 16 rows and walks 64-column tiles, a rating workgroup takes 16 rows with 16 lanes each,
so N = 1, 2, 3 (N < k2), 7 (N < k1), 12, 64, 65, 129 (the special pairs; the first interior tiles, stored entry by entry
pair-wise because N is odd), 130 (the same with 16-byte stores), 513 (several row blocks, edge tiles in both directions) and
1600 (past the 1536 lines the rating stages in LDS: bit for bit against the EM's pair pass)."""
import ctypes
import functools

import numpy as np
import pytest

import em_phase_reference as E
import line_geometry_reference as R

pytestmark = pytest.mark.gpu

VPK_ERR_ARG = -1
SENTINEL = -7.25


def _rt():
    from vanishing_points_2017_amd.runtime import get_runtime
    return get_runtime(0)


def _V():
    from vanishing_points_2017_amd import vp_localisation
    return vp_localisation


def _dev(a, dtype=np.float64):
    rt = _rt()
    return rt.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(rt.tdev)


def _i64(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _cat(sizes):
    offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    return np.ascontiguousarray(np.concatenate([R.case(n) for n in sizes])), offsets


def raw_similarity(lp, offsets, sigma, mat, batch=None):
    """The C entry on sentinel-filled output: (return code, lsim buffer)."""
    rt = _rt()
    offsets, po = _i64(offsets)
    mat, pm = _i64(mat)
    with rt.on_stream():
        d_lp = _dev(lp)
        out = rt.torch.full((max(int(mat.max()), 1),), SENTINEL, dtype=rt.torch.float64, device=rt.tdev)
        rc = rt.lib.vpk_line_similarity_batch(rt.h, len(offsets) - 1 if batch is None else batch, po, rt.ptr(d_lp), float(sigma),
                                              pm, rt.ptr(out))
    rt.synchronize()
    return rc, out.cpu().numpy()


def raw_rating(lp, offsets, k1, k2, sigma, want=(True, True, True), batch=None):
    rt = _rt()
    offsets, po = _i64(offsets)
    with rt.on_stream():
        d_lp = _dev(lp)
        outs = [rt.torch.full((max(int(offsets.max()), 1),), SENTINEL, dtype=rt.torch.float64, device=rt.tdev) if w else None
                for w in want]
        rc = rt.lib.vpk_line_rating_batch(rt.h, len(offsets) - 1 if batch is None else batch, po, rt.ptr(d_lp), int(k1), int(k2),
                                          float(sigma), rt.ptr(outs[0]), rt.ptr(outs[1]), rt.ptr(outs[2]))
    rt.synchronize()
    return rc, [None if o is None else o.cpu().numpy() for o in outs]


@functools.lru_cache(maxsize=None)
def pairwise(n):
    from vanishing_points_2017_amd import kernels
    return kernels.pairwise(np.array(R.case(n)))


@pytest.mark.parametrize("n", R.SHAPES + (130,))
def test_similarity_meets_the_bars(n):
    lp = np.array(R.case(n))
    for sigma in R.SIM_SIGMAS:
        lsim = _V().calc_lsim(lp, sigma=sigma)
        R.check_lsim(lsim, n, sigma)
    assert np.array_equal(lp, R.case(n))
    assert np.array_equal(_V().calc_lsim(lp), _V().calc_lsim(lp, sigma=0.1))       # the reference's default (:87)


@pytest.mark.parametrize("n", R.SHAPES)
def test_rating_meets_the_bars(n):
    lp = np.array(R.case(n))
    V = _V()
    for sigma in R.RATING_SIGMAS:
        for k1, k2 in R.KNN:
            R.check_lscore(V.line_rating_knn(lp, k1=k1, k2=k2, sigma=sigma), n, k1, k2, sigma)
    assert np.array_equal(V.line_rating_knn(lp), V.line_rating_knn(lp, k1=10, k2=3, sigma=1))    # the defaults of :34
    lscore, langle, llen, offsets = V.line_geometry_batch([lp])
    assert list(offsets) == [0, n]
    R.check_angles(langle.cpu().numpy(), llen.cpu().numpy(), n)
    assert np.array_equal(lscore.cpu().numpy(), V.line_rating_knn(lp))
    assert np.array_equal(langle.cpu().numpy(), V.lines_angles(lp))
    assert np.array_equal(lp, R.case(n))


@pytest.mark.parametrize("n", (12, 129, 513, 1600))
def test_bit_equal_with_the_em_pair_pass(n):
    """At the EM's settings (sigma = 1, k1 = 10, k2 = 4) the three outputs are vpk_pairwise's."""
    lp = np.array(R.case(n))
    lsim, lscore, langle = pairwise(n)
    V = _V()
    got = V.calc_lsim(lp, sigma=1)
    assert np.array_equal(got, lsim, equal_nan=True)
    assert np.array_equal(got, got.T, equal_nan=True) and (np.diagonal(got) == 0).all()
    assert np.array_equal(V.line_rating_knn(lp, k1=10, k2=4, sigma=1), lscore, equal_nan=True)
    assert np.array_equal(V.lines_angles(lp), langle, equal_nan=True)


def test_ragged_batch_is_the_single_images():
    """[0, 1, 12, 129, 65] in one launch: image b equals the single-image call bit for bit; the padding between matrices,
    the rows of NULL outputs and an empty image's slots keep the sentinel."""
    sizes = list(R.RAGGED)
    lp, offsets = _cat(sizes)
    V = _V()
    pad = 5
    mat = np.concatenate(([0], np.cumsum([n * n + pad for n in sizes]))).astype(np.int64)
    rc, buf = raw_similarity(lp, offsets, 0.1, mat)
    assert rc == 0
    rc, (lscore, langle, llen) = raw_rating(lp, offsets, 10, 3, 1.0)
    assert rc == 0
    rc, (no_score, only_angle, no_len) = raw_rating(lp, offsets, 10, 3, 1.0, want=(False, True, False))
    assert rc == 0 and no_score is None and no_len is None and np.array_equal(only_angle, langle)
    rc, (only_score, _, _) = raw_rating(lp, offsets, 10, 3, 1.0, want=(True, False, False))
    assert rc == 0 and np.array_equal(only_score, lscore)
    singles = []
    for b, n in enumerate(sizes):
        assert (buf[mat[b] + n * n:mat[b + 1]] == SENTINEL).all(), "padding behind matrix %d was written" % b
        if n == 0:
            singles.append(None)
            continue
        one = V.calc_lsim(np.array(R.case(n)), sigma=0.1)
        singles.append(one)
        assert np.array_equal(buf[mat[b]:mat[b] + n * n].reshape(n, n), one)
        sl = slice(offsets[b], offsets[b + 1])
        s1, a1, l1, _ = V.line_geometry_batch([np.array(R.case(n))])
        assert np.array_equal(lscore[sl], s1.cpu().numpy())
        assert np.array_equal(langle[sl], a1.cpu().numpy()) and np.array_equal(llen[sl], l1.cpu().numpy())
    # the Python batch forms: a list of arrays, and a device tensor with host offsets
    rt = _rt()
    for lps in ([np.array(R.case(n)) for n in sizes], (_dev(lp), offsets)):
        mats = V.calc_lsim_batch(lps)
        assert [tuple(m.shape) for m in mats] == [(n, n) for n in sizes]
        assert all(m.device == rt.tdev and m.dtype == rt.torch.float64 for m in mats)
        for m, one in zip(mats, singles):
            assert one is None or np.array_equal(m.cpu().numpy(), one)
        assert len({m.untyped_storage().data_ptr() for m in mats}) == 1          # views into one allocation
        s, a, l, off = V.line_geometry_batch(lps)
        assert np.array_equal(off, offsets)
        assert np.array_equal(s.cpu().numpy(), lscore) and np.array_equal(a.cpu().numpy(), langle)
        assert np.array_equal(l.cpu().numpy(), llen)


def test_empty_batches_do_nothing():
    lp, offsets = _cat([12])
    rc, buf = raw_similarity(lp, [0], 0.1, [0], batch=0)
    assert rc == 0 and (buf == SENTINEL).all()
    rc, outs = raw_rating(lp, [0], 10, 3, 1.0, batch=0)
    assert rc == 0 and all((o == SENTINEL).all() for o in outs)
    rc, buf = raw_similarity(lp, [0, 0, 0], 0.1, [0, 3, 3])
    assert rc == 0 and (buf == SENTINEL).all()
    rc, outs = raw_rating(lp, [0, 0, 0], 10, 3, 1.0)
    assert rc == 0 and all((o == SENTINEL).all() for o in outs)
    V = _V()
    assert V.calc_lsim_batch([]) == []
    assert [tuple(m.shape) for m in V.calc_lsim_batch([np.zeros((0, 4))])] == [(0, 0)]
    s, a, l, off = V.line_geometry_batch([np.zeros((0, 4))])
    assert s.numel() == a.numel() == l.numel() == 0 and list(off) == [0, 0]


def test_argument_errors_leave_the_outputs_untouched():
    lp, offsets = _cat([12, 7])
    mat = [0, 144, 193]
    bad_sim = [dict(batch=-1), dict(offsets=[0, 12, 5]), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
               dict(mat=[0, 143, 193]), dict(mat=[0, 144, 192])]
    for kw in bad_sim:
        rc, buf = raw_similarity(lp, kw.get("offsets", offsets), kw.get("sigma", 0.1), kw.get("mat", mat), batch=kw.get("batch"))
        assert rc == VPK_ERR_ARG, kw
        assert (buf == SENTINEL).all(), kw
    bad_rate = [dict(batch=-1), dict(offsets=[0, 12, 5]), dict(sigma=0.0), dict(sigma=-2.0), dict(sigma=float("nan")),
                dict(k1=0, k2=0), dict(k1=17), dict(k1=-3), dict(k2=0), dict(k1=3, k2=4), dict(k1=16, k2=17)]
    for kw in bad_rate:
        rc, outs = raw_rating(lp, kw.get("offsets", offsets), kw.get("k1", 10), kw.get("k2", 3), kw.get("sigma", 1.0),
                              batch=kw.get("batch"))
        assert rc == VPK_ERR_ARG, kw
        assert all((o == SENTINEL).all() for o in outs), kw
    assert "vpk_line_rating_batch" in _rt().lib.vpk_last_error(_rt().h).decode()
    # the good call right after: the handle is usable
    rc, outs = raw_rating(lp, offsets, 16, 16, 1.0)
    assert rc == 0 and not any((o == SENTINEL).any() for o in outs)


def test_thin_mirrors_are_the_fine_grained_entries():
    from vanishing_points_2017_amd import kernels
    V = _V()
    cnn, sphere = E.init_case(500, 25, "few")
    v0, _ = kernels.init_vps(cnn, sphere, num_max=25)
    got = V.find_initial_vps(sphere, cnn, 25)
    assert v0.shape[0] > 0 and got.shape == v0.shape and np.array_equal(got, v0)
    cnn, sphere = E.init_case(500, 25, "blank")
    with pytest.raises(ValueError, match="need at least one array"):
        V.find_initial_vps(sphere, cnn, 25)                                       # np.vstack([]) at :165

    rs = np.random.RandomState(7)
    lp = np.array(R.case(12))
    p_vl, lweight = rs.rand(3, 12), rs.rand(12)
    lsim = V.calc_lsim(lp)
    assert np.array_equal(V.weight_matrix(p_vl, lweight, lsim), kernels.weight_matrix(p_vl, lweight, lsim, bias=0.001))
    assert np.array_equal(V.weight_matrix(p_vl, lweight, lsim, bias=0.5), kernels.weight_matrix(p_vl, lweight, lsim, bias=0.5))

    l = rs.randn(12, 3)
    l /= np.linalg.norm(l, axis=1)[:, None]
    w = rs.rand(12)
    vp, valid = kernels.mstep(l, w[None, :])
    got = V.calc_new_vanishing_point(l, w)
    assert valid[0] and got.shape == (3,) and np.array_equal(got, vp[0])
    assert abs(np.linalg.norm(got) - 1) < 1e-12
    _, valid = kernels.mstep(l, np.zeros((1, 12)))
    assert not valid[0]
    assert V.calc_new_vanishing_point(l, np.zeros(12)) is None                    # :459-460
    assert V.calc_new_vanishing_point(np.zeros((0, 3)), np.zeros(0)) is None      # :456-457
