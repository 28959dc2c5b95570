"""csrc/train_plan.hpp -- what the two training drivers (vpk_train.hip, vpk_convtrain.hip) decide on the host: the head's launch
plans and workspace sizes, the conv stack's shapes, limits and buffers, the kept blobs' life cycle, the solver's rates and the
set_params rules -- compiled for the host by tests/hostsim/sim_train_plan.cpp.  The expectations are written out here from
the rules (and from tests/convtrain_reference.py, tests/train_reference.py), not read back from the header.  CPU only: no
GPU, no libvpk.so."""
import itertools

import numpy as np
import pytest

import convtrain_reference as C
import train_reference as R
from hostsim import simlib_convtrain
from hostsim import simlib_train_plan as sim

NS, KS = (1, 7, 16, 17, 400), (1, 4, 255, 256, 257, 4096)
GRID = list(itertools.product(NS, KS))
BATCHES = (1, 8, 9, 32)


def ceil_div(a, b):
    return -(-a // b)


def test_constants():
    assert sim.constants() == dict(TRAIN_MAX_B=32, FWD_RT=16, SWEEP_KT=256, SWEEP_MIN_RT=16, SWEEP_MAX_RT=128, CT_MAX_B=32,
                                   CT_MAX_LAYERS=32, CT_TILE=64, CT_LRN_PIX=32, CT_LRN_MAX_C=512,
                                   sizes=(48, 44))                       # include/vpk.h's two structures


# ---- the head ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k, rt, tiles, slabs, per_slab, row_tiles", [
    # fc6: 225 column tiles; 4096 * 225 / 2048 = 450 rows, capped at 128.  Forward: 256 row tiles, 2048 / 256 = 8 slabs of
    # ceil(225 / 8) = 29 chunks, and 8 slabs of 29 still cover 225
    (4096, 57600, 128, 32, 8, 29, 256),
    # fc7: 16 column tiles; 4096 * 16 / 2048 = 32 rows.  Forward: 8 slabs of 2 of the 16 chunks
    (4096, 4096, 32, 128, 8, 2, 256),
    # fc8: 400 * 16 / 2048 -> 4 -> 8 rows, raised to 16.  Forward: 25 row tiles, 82 slabs wanted, 16 chunks to deal
    (400, 4096, 16, 25, 16, 1, 25)])
def test_head_plan_at_the_net(n, k, rt, tiles, slabs, per_slab, row_tiles):
    assert sim.sweep(n, k) == (rt, tiles, ceil_div(k, 256))
    assert sim.fwd(n, k) == (ceil_div(k, 256), per_slab, slabs, row_tiles)


@pytest.mark.parametrize("n, k", GRID)
def test_head_plan_covers(n, k):
    rt, tiles, col_tiles = sim.sweep(n, k)
    assert rt % 8 == 0 and 16 <= rt <= 128
    assert (tiles - 1) * rt < n <= tiles * rt, "the tiles cover N and none is empty"
    assert (col_tiles - 1) * 256 < k <= col_tiles * 256
    chunks, per_slab, slabs, row_tiles = sim.fwd(n, k)
    assert (chunks - 1) * 256 < k <= chunks * 256 and (row_tiles - 1) * 16 < n <= row_tiles * 16
    # the kernel's slab s takes chunks [s per_slab, min((s + 1) per_slab, chunks))
    taken = [c for s in range(slabs) for c in range(s * per_slab, min((s + 1) * per_slab, chunks))]
    assert taken == list(range(chunks)), "every chunk exactly once"
    assert all(s * per_slab < chunks for s in range(slabs)), "no slab is empty"
    assert slabs == chunks or 2048 <= slabs * row_tiles < 2048 + row_tiles, "one slab per chunk, or the target of workgroups"


def test_vec_and_nb():
    for k in KS + (8, 57600):
        for low in itertools.product((0, 4, 8, 16), repeat=3):
            ptrs = [0x7f0000001000 + v for v in low]
            assert sim.vec(k, ptrs) == (k % 4 == 0 and all(v % 16 == 0 for v in low)), (k, low)
            assert sim.vec(k, ptrs + [0]) == sim.vec(k, ptrs), "a pointer the launch does not use"
            assert sim.vec(k, ptrs + [0x7f0000002004]) is False
    assert [sim.nb(b) for b in range(1, 33)] == [8] * 8 + [32] * 24


@pytest.mark.parametrize("n, k", GRID)
def test_head_workspaces_hold_every_launch(n, k):
    """the highest element each launch of a step writes or reads, from the plan: the forward's partial[slab][b][n], a sweep's
    partial[row tile][b][k]"""
    for dims in ((k, n, 3, 5), (2, k, n, 5), (2, 3, k, n)):          # the n x k layer as fc6, as fc7 and as fc8
        for b in BATCHES:
            partial, fpartial, xpartial = sim.workspaces(dims, b)
            for l in range(3):
                ln, lk = dims[l + 1], dims[l]
                assert sim.fwd(ln, lk)[2] * b * ln * 4 <= fpartial
                if l > 0:
                    assert sim.sweep(ln, lk)[1] * b * lk * 4 <= partial
            assert xpartial == sim.sweep(dims[1], dims[0])[1] * b * dims[0] * 4
        assert partial == 4 * 32 * max(sim.sweep(dims[2], dims[1])[1] * dims[1], sim.sweep(dims[3], dims[2])[1] * dims[2])


# ---- the conv stack ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_shape, stack", [(C.EDGE_SHAPE, C.EDGE_STACK), (C.NET_SHAPE, C.NET_STACK)])
def test_stack_shapes(in_shape, stack):
    assert sim.chain(in_shape, stack) == (sim.OK, C.shapes(in_shape, stack))
    assert C.shapes(C.NET_SHAPE, C.NET_STACK)[-1] == (256, 15, 15)


def test_stack_refusals():
    bad = [[C.pool(k=3)], [C.conv(4, 7)], [C.conv(4, 3, groups=3)], [C.conv(6, 3, groups=4)], [C.lrn(n=4)],
           [C.conv(4, 3, stride=0)], [C.conv(4, 3, pad=1), C.pool(), C.pool(), C.pool(k=3)]]      # test_gpu_convtrain.py's
    for layers in bad:
        shape = (2, 6, 5) if layers[0].get("groups", 1) > 1 else (1, 2, 6)
        assert sim.chain(shape, layers)[0] == sim.NO_CHAIN, layers
    assert sim.chain((2, 6, 5), [])[0] == sim.NO_CHAIN
    assert sim.chain((0, 6, 5), [C.lrn()])[0] == sim.NO_CHAIN
    assert sim.chain((2, 6, 5), [sim.StackLayer(kind=3)])[0] == sim.NO_CHAIN
    assert sim.chain((513, 2, 2), [C.lrn()])[0] == sim.LRN_WIDE
    assert sim.chain((512, 2, 2), [C.lrn()])[0] == sim.OK
    assert sim.chain((513, 2, 2), [C.lrn(), C.pool(k=3)])[0] == sim.NO_CHAIN, "a chain that breaks is that first"
    assert sim.chain((1, 2, 2), [C.lrn()] * 32)[0] == sim.OK
    assert sim.chain((1, 2, 2), [C.lrn()] * 33)[0] == sim.NO_CHAIN


def test_stack_index_limit():
    """OC OH OW of 32 images must index in int: 2^26 elements per image are refused, 2^26 - 1 = 3 * 2731 * 8191 accepted"""
    assert 3 * 2731 * 8191 == 2 ** 26 - 1
    assert sim.chain((1, 2731, 8191), [C.conv(3, 1)]) == (sim.OK, [(3, 2731, 8191)])
    assert sim.chain((1, 8192, 8192), [C.conv(1, 1)])[0] == sim.NO_CHAIN
    assert sim.chain((1, 8192, 8192), [C.conv(1, 1, stride=2)])[0] == sim.OK
    assert sim.chain((1, 2731, 8191), [C.conv(3, 1), C.lrn()])[0] == sim.OK
    assert sim.chain((1, 2731, 8191), [C.conv(3, 1), C.conv(4, 1)])[0] == sim.NO_CHAIN, "any layer's output"


@pytest.mark.parametrize("in_shape, stack", [(C.EDGE_SHAPE, C.EDGE_STACK), (C.NET_SHAPE, C.NET_STACK)])
def test_stack_buffers_and_grids(in_shape, stack):
    shapes = C.shapes(in_shape, stack)
    wshapes = iter(C.weight_shapes(in_shape, stack))
    for b in (1, 5, 32):
        want, cur = 0, in_shape
        for l, d in enumerate(stack):
            p = sim.layer_plan(in_shape, stack, l, b)
            oc, oh, ow = shapes[l]
            assert p["blob_bytes"] == b * oc * oh * ow * 4
            if d["kind"] == "conv":
                icg, ocg = cur[0] // d["groups"], oc // d["groups"]
                slabs, slab_len = simlib_convtrain.wgrad_slabs((b,) + tuple(cur), d)      # convtrain_device.hpp's own split
                cols = icg * d["k"] * d["k"] + 1
                assert (p["slabs"], p["slab_len"], p["cols"]) == (slabs, slab_len, cols)
                assert p["wgrad_bytes"] == slabs * oc * cols * 4
                want = max(want, p["wgrad_bytes"])
                assert p["grid"][sim.FWD] == [ceil_div(b * oh * ow, 64), ceil_div(ocg, 64), d["groups"]]
                assert p["grid"][sim.DGRAD] == [ceil_div(b * cur[1] * cur[2], 64), ceil_div(icg, 64), d["groups"]]
                assert p["grid"][sim.WGRAD] == [ceil_div(cols, 64), ceil_div(ocg, 64), d["groups"] * slabs]
                if b == 1:
                    assert p["weights"] == int(np.prod(next(wshapes))) and next(wshapes) == (oc,)
            if d["kind"] == "lrn":
                assert p["lrn_grid"] == [ceil_div(cur[1] * cur[2], 32), b] and p["lrn_lds"] == cur[0] * 32 * 4 <= 65536
            cur = shapes[l]
        assert sim.slab_buffer(in_shape, stack, b) == want > 0
    assert sim.slab_buffer((3, 9, 9), [C.pool(), C.lrn()], 5) == 0, "a stack without CONV layers needs none"


# ---- the kept blobs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("events, backward, read, gradient, batch", [
    ([], False, False, False, 0),                      # nothing yet: a read, a gradient read and a backward are refused
    ([0, 5], True, True, False, 5),                    # a forward: a gradient read is refused before a backward
    ([0, 5, -1], False, True, True, 5),                # a backward consumes it: a second one is refused, the outputs stay
    ([0, 5, -1, 0], False, False, False, 0),           # a forward that was refused after it began to launch: nothing is kept
    ([0, 5, 0], False, False, False, 0),
    ([0, 5, -1, 0, 2], True, True, False, 2),          # the next forward: the gradients are no longer its own
    ([0, 5, 0, 3, -1], False, True, True, 3)])
def test_kept_blobs(events, backward, read, gradient, batch):
    got = sim.kept(events)
    assert got[:3] == (backward, read, gradient)
    assert got[3] == (batch if backward else 0) and got[4] == batch


# ---- the solver -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("changed", [{}, {"gamma": 0.5, "stepsize": 3}])
def test_rates(changed):
    """to the bit: train_reference's float32 chain of the learning rate times the multipliers"""
    p = sim.params(**changed)
    ref = dict(R.DEFAULTS, **changed)
    for it in (0, 2, 3, 6, 200000):
        lr = R.learning_rate32(ref, it)
        f = np.float32
        want = np.array([lr * f(ref["lr_mult_weight"]), f(ref["weight_decay"]) * f(ref["decay_mult_weight"]),
                         lr * f(ref["lr_mult_bias"]), f(ref["weight_decay"]) * f(ref["decay_mult_bias"]), f(ref["momentum"])],
                        dtype=np.float32)
        got = sim.rates(p, it)
        assert got.tobytes() == want.tobytes(), (it, got, want)
        assert np.array_equal(got.astype(np.float64), np.array(R.local_rates(ref, it)[:5]))
    assert sim.rates(sim.params(gamma=0.5, stepsize=3), 6)[0] == np.float32(1e-4) * np.float32(0.25)


def test_set_params_rules():
    """the head divides by 1 - dropout_ratio and refuses ratios outside [0, 1); the stack ignores the ratio"""
    for ratio, head in ((-0.1, False), (0.0, True), (0.999, True), (1.0, False), (float("nan"), False)):
        assert sim.params_ok(sim.params(dropout_ratio=ratio), head=True) is head, ratio
        assert sim.params_ok(sim.params(dropout_ratio=ratio), head=False) is True, ratio
    for head in (True, False):
        assert sim.params_ok(sim.params(stepsize=0), head) is False
        assert sim.params_ok(sim.params(stepsize=1), head) is True
