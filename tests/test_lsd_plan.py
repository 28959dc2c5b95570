"""csrc/lsd_plan.hpp -- what vpk_lsd_detect_batch (vpk_lsd_gpu.hip) decides on the host before it launches: the rules a
batch's images are held to, every image's slice of the workspace and the chunks under the workspace limit -- compiled for
the host by tests/hostsim/sim_lsd_plan.cpp, each rule and the limit at their edges.  CPU only: no GPU, no libvpk.so."""
import ctypes
import math

import numpy as np
import pytest

from hostsim import hostbuild

OK, SIDE, OFFSETS, DIM, PIXELS = range(5)                            # PlanRule, in the order the driver checks an image
VPK_OK, VPK_ERR_ARG, VPK_ERR_LIMIT = 0, -1, -5                       # include/vpk.h
META = 16                                                            # sizeof(Meta)
ARRAYS = ("aux", "scaled", "ang", "grad", "order", "reg", "used")


@pytest.fixture(scope="module")
def sim():
    lib = hostbuild.load("lsd_plan")
    lib.sim_lsd_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_ulonglong] + \
        [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 3
    assert lib.sim_lsd_plan_meta_bytes() == META
    return lib


def plan(sim, shapes, scale=1.0, limit=0, offsets=None):
    """shapes: (width, height) per image -> (rule, image) when the batch is refused, else a dict: per array name the
    offsets of every image, xs, ys, starts, ws_bytes, max_c."""
    batch = len(shapes)
    dims = np.array(shapes, dtype=np.int32).reshape(-1, 2)
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum(dims[:, 0].astype(np.int64) * dims[:, 1])))
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    assert off.shape == (batch + 1,)
    image, n_starts, max_c = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    ws = ctypes.c_ulonglong(0)
    o, geom, starts = np.full((batch, 7), -7, np.int64), np.full((batch, 2), -7, np.int32), np.full(batch + 1, -7, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rule = sim.sim_lsd_plan(batch, p(dims), p(off), scale, limit, ctypes.byref(image), p(o), p(geom), p(starts), batch + 1,
                            ctypes.byref(n_starts), ctypes.byref(ws), ctypes.byref(max_c))
    assert rule >= 0, "a descriptor does not carry its image's index, size or first pixel"
    if rule != OK:
        return rule, image.value
    res = {name: o[:, k] for k, name in enumerate(ARRAYS)}
    res.update(xs=geom[:, 0], ys=geom[:, 1], starts=starts[:n_starts.value].tolist(), ws_bytes=ws.value, max_c=max_c.value)
    return res


def test_layout_of_one_image(sim):
    r = plan(sim, [(8, 8)])
    # Meta block, then ang 64 * 8, grad 64 * 8, order 64 * 4 -> 256, reg 64 * 8, used 64 -> 256: 2 048 bytes
    assert [int(r[a][0]) for a in ARRAYS] == [0, 0, 256, 768, 1280, 1536, 2048]
    assert r["ws_bytes"] == 256 + 512 + 512 + 256 + 512 + 256 == 256 + 2048
    assert (r["xs"][0], r["ys"][0], r["max_c"], r["starts"]) == (8, 8, 0, [0, 1])      # no Gaussian weights at scale 1
    r = plan(sim, [(8, 8)], scale=0.8)
    # xs = ys = ceil(6.4) = 7; aux 7 * 8 samples * 8 -> 512, scaled 49 * 8 -> 512, ang, grad 512, order 196 -> 256, reg 512,
    # used 49 -> 256
    assert [int(r[a][0]) for a in ARRAYS] == [256, 768, 1280, 1792, 2304, 2560, 3072]
    assert r["ws_bytes"] == 3328 and (r["xs"][0], r["ys"][0], r["max_c"]) == (7, 7, 7)
    r = plan(sim, [(9, 13)], scale=0.8)                       # aux covers xs * height: 8 * 13 * 8 = 832 -> 1 024
    assert (r["xs"][0], r["ys"][0], r["max_c"]) == (8, 11, 11)
    assert r["scaled"][0] - r["aux"][0] == 1024 and r["ang"][0] - r["scaled"][0] == 768


def test_chunks_hold_at_most_4096_images(sim):
    r = plan(sim, [(8, 8)] * 4097)
    assert r["starts"] == [0, 4096, 4097]
    assert r["ws_bytes"] == 65536 + 4096 * 2048 == 8454144
    assert r["ang"][0] == 65536 and r["ang"][4095] == 65536 + 4095 * 2048
    assert r["ang"][4096] == 256, "the second chunk starts again after its own Meta block"


def test_the_limit_at_its_edge(sim):
    two = [(8, 8)] * 2
    assert plan(sim, two, limit=4352)["starts"] == [0, 2]      # 256 bytes of Meta plus two images of 2 048
    assert plan(sim, two, limit=4352)["ws_bytes"] == 4352
    r = plan(sim, two, limit=4351)
    assert r["starts"] == [0, 1, 2] and r["ws_bytes"] == 2304 and list(r["ang"]) == [256, 256]
    assert plan(sim, two, limit=1)["starts"] == [0, 1, 2], "one image per chunk, never an empty chunk"
    assert plan(sim, [(8, 8)] * 5, limit=1)["starts"] == [0, 1, 2, 3, 4, 5]


def _sizes(w, h, xs, ys):
    """bytes of the seven arrays of one image, from the kernels' indexing"""
    P = xs * ys
    return [xs * h * 8, P * 8, P * 8, P * 8, P * 4, P * 8, P]


RAGGED = [(8, 8), (9, 13), (48, 40), (96, 80), (33, 17)]


def _image_bytes(w, h, scale):
    xs, ys = (math.ceil(w * scale), math.ceil(h * scale)) if scale != 1.0 else (w, h)
    return sum((s + 255) // 256 * 256 for s in _sizes(w, h, xs, ys)[(0 if scale != 1.0 else 2):])


@pytest.mark.parametrize("scale", [0.8, 1.0])
@pytest.mark.parametrize("chunks", [1, 2, 5])
def test_offsets_across_chunks(sim, scale, chunks):
    b = [_image_bytes(w, h, scale) for w, h in RAGGED]
    assert b[0] + b[1] + b[2] > b[4]
    # 2 chunks: the limit holds images 3 and 4 behind their Meta block, so images 0..2 fit and image 3 does not join them
    limit = {1: 0, 2: 256 + b[3] + b[4], 5: 1}[chunks]
    r = plan(sim, RAGGED, scale=scale, limit=limit)
    assert r["starts"] == {1: [0, 5], 2: [0, 3, 5], 5: [0, 1, 2, 3, 4, 5]}[chunks]
    ends = []
    for s, e in zip(r["starts"][:-1], r["starts"][1:]):
        spans = [(0, (e - s) * META)]                          # the chunk's Meta array at the workspace's first byte
        for k in range(s, e):
            w, h = RAGGED[k]
            assert (r["xs"][k], r["ys"][k]) == ((math.ceil(w * scale), math.ceil(h * scale)) if scale != 1.0 else (w, h))
            sizes = _sizes(w, h, int(r["xs"][k]), int(r["ys"][k]))
            for a, size in list(zip(ARRAYS, sizes))[(0 if scale != 1.0 else 2):]:
                assert r[a][k] % 256 == 0
                spans.append((int(r[a][k]), int(r[a][k]) + size))
            if scale == 1.0:
                assert r["aux"][k] == 0 and r["scaled"][k] == 0
        assert spans[1][0] == ((e - s) * META + 255) // 256 * 256, "the first image follows the chunk's own Meta block"
        assert [x[0] for x in spans] == sorted(x[0] for x in spans), "aux, scaled, ang, grad, order, reg, used, image by image"
        for (a0, a1), (b0, b1) in zip(spans[:-1], spans[1:]):
            assert a0 < a1 <= b0, "two arrays of a chunk overlap"
        assert spans[-1][1] <= r["ws_bytes"]
        ends.append((spans[-1][1] + 255) // 256 * 256)
    assert r["ws_bytes"] == max(ends)
    assert r["max_c"] == (max(max(r["xs"]), max(r["ys"])) if scale != 1.0 else 0)


def test_refusals_each_followed_by_an_accepted_call(sim):
    good = [(8, 8), (20, 30)]

    def accepted():
        assert plan(sim, good)["starts"] == [0, 2]

    assert plan(sim, [(8, 8), (7, 30)]) == (SIDE, 1) and plan(sim, [(30, 7)]) == (SIDE, 0)
    accepted()
    for off in ([0, 64, 663], [0, 64, 665], [0, 63, 664], [-64, 0, 600]):     # one short, one long, negative
        rule, image = plan(sim, good, offsets=off)
        assert rule == OFFSETS and image == (0 if off[0] < 0 or off[1] != 64 else 1), off
        accepted()
    assert plan(sim, good, offsets=[5, 69, 669])["starts"] == [0, 2], "a batch may be a window of a longer array"
    side = 1 << 20
    assert plan(sim, [(8, 8), (side + 1, 8)]) == (DIM, 1) and plan(sim, [(8, side + 1)]) == (DIM, 0)
    accepted()
    assert plan(sim, [(side, 8)], scale=1.25) == (DIM, 0) and plan(sim, [(8, side)], scale=1.25) == (DIM, 0)
    r = plan(sim, [(side, 8)])
    assert r["starts"] == [0, 1] and r["xs"][0] == side
    assert plan(sim, [(32768, 32769)]) == (PIXELS, 0)
    r = plan(sim, [(32768, 32768)])                            # 2^30 pixels plan, and planning allocates no workspace
    assert r["starts"] == [0, 1] and r["ws_bytes"] == 256 + (8 + 8 + 4 + 8 + 1) * (1 << 30)
    accepted()


def test_the_earlier_rule_is_reported(sim):
    side = 1 << 20
    assert plan(sim, [(7, 30)], offsets=[0, 1]) == (SIDE, 0)                       # side and offsets
    assert plan(sim, [(side + 1, 8)], offsets=[0, 1]) == (OFFSETS, 0)              # offsets and side limit
    assert plan(sim, [(7, side + 1)]) == (SIDE, 0)                                 # side and side limit
    assert plan(sim, [(side, side)], scale=1.25) == (DIM, 0)                       # side limit and pixel limit
    # image by image: an earlier image's later rule comes before a later image's earlier rule
    assert plan(sim, [(32768, 32769), (7, 30)]) == (PIXELS, 0)
    assert plan(sim, [(8, 8), (32768, 32769), (7, 30)], offsets=[0, 64, 64 + 32768 * 32769, 0]) == (PIXELS, 1)


def test_codes(sim):
    want = {OK: VPK_OK, SIDE: VPK_ERR_ARG, OFFSETS: VPK_ERR_ARG, DIM: VPK_ERR_LIMIT, PIXELS: VPK_ERR_LIMIT}
    for rule, code in want.items():
        assert sim.sim_lsd_plan_code(rule) == code
