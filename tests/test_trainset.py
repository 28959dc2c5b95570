"""The device-resident training set without a GPU: the host build of csrc/trainset_device.hpp (tests/hostsim/
sim_trainset.cpp) against the NumPy / Python-integer restatement (tests/trainset_reference.py), train.Augment's transforms,
train.TrainSet's orders, train.Solver's schedule on stubs, and the solver's defaults against the prototxts' numbers."""
import inspect
import json
import os

import numpy as np
import pytest

import trainset_reference as T
from hostsim import simlib_trainset as S
from vanishing_points_2017_amd import _lib, train

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def test_draws_equal_python():
    for seed in (0, 1, 2 ** 63 + 5):
        for iteration in (0, 1, 399999, 2 ** 40):
            for b in (0, 4, 31):
                got = S.draws(seed, iteration, b, 6)
                want = np.array([T.draw(seed, iteration, b, k) for k in range(6)])
                assert got.tobytes() == want.tobytes(), (seed, iteration, b)
                assert np.array_equal(train.draws(seed, iteration, b, 6), want)
                assert ((got >= 0) & (got < 1)).all()
    assert not np.array_equal(S.draws(0, 0, 0, 6), S.draws(0, 0, 1, 6))
    assert not np.array_equal(S.draws(0, 0, 0, 6), S.draws(0, 1, 0, 6))
    assert not np.array_equal(S.draws(0, 0, 0, 6), S.draws(1, 0, 0, 6))


def test_order_keys_equal_python():
    for seed, epoch in ((0, 0), (3, 2 ** 40)):
        k0 = T.mask_key(seed, epoch, 0x53, 0)
        want = np.array([T.mix64(k0 ^ i) for i in range(50)], dtype=np.uint64)
        assert np.array_equal(S.order_keys(seed, epoch, 50), want)


def _random_cases(n, seed):
    rs = np.random.RandomState(seed)
    h = rs.standard_normal((n, 6)) * np.exp(rs.uniform(-3, 3, (n, 1)))
    l = rs.standard_normal((n, 3)) * np.exp(rs.uniform(-3, 3, (n, 1)))
    v = rs.standard_normal((n, 3)) * np.exp(rs.uniform(-3, 3, (n, 1)))
    return h, l, v


def test_transforms_equal_numpy():
    h, l, v = _random_cases(1000, 11)
    m, w = S.transform(h, l, v)
    assert m.tobytes() == T.transform_lines(h, l).tobytes()
    assert w.tobytes() == T.transform_vps(h, v).tobytes()
    assert all(S.valid(row) for row in h)
    for special in (IDENTITY, (-1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.25, 0.0, 1.0, -0.125)):
        hs = np.tile(np.array(special), (1000, 1))
        m, w = S.transform(hs, l, v)
        assert m.tobytes() == T.transform_lines(hs, l).tobytes(), special
        assert w.tobytes() == T.transform_vps(hs, v).tobytes(), special
        assert S.valid(hs[0])
    m, w = S.transform(np.tile(np.array(IDENTITY), (1000, 1)), l, v)
    assert np.array_equal(m, l) and np.array_equal(w, v)             # the identity in value
    hs = np.tile(np.array((-1.0, 0.0, 0.0, 0.0, 1.0, 0.0)), (1000, 1))
    m, w = S.transform(hs, l, v)                                     # the mirror x -> -x: det < 0, the line up to the sign
    assert np.array_equal(w, v * np.array([-1.0, 1.0, 1.0])) and np.array_equal(m, l * np.array([1.0, -1.0, -1.0]))


def test_transformed_lines_pass_through_transformed_points():
    """the formulas mean what they say: a point on l maps to a point on the transformed line, H v of a VP of l lies on it"""
    rs = np.random.RandomState(5)
    h = train.Augment(0.4, 1.5, 0.2, 0.5).transforms(9, 3, 64)
    p, q = rs.uniform(-1, 1, (64, 3)), rs.uniform(-1, 1, (64, 3))
    l = np.cross(p, q)
    m = T.transform_lines(h, l)
    for x in (p, q):
        res = np.abs(np.sum(m * T.transform_vps(h, x), 1))
        assert (res <= 1e-13 * np.linalg.norm(m, axis=1) * np.linalg.norm(x, axis=1) * 4).all()


def test_validity():
    assert S.valid(IDENTITY)
    assert not S.valid((1.0, 2.0, 0.0, 2.0, 4.0, 0.0))                                   # det == 0
    assert not S.valid((0.0, 0.0, 0.0, 0.0, 0.0, 0.0))
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            h = list(IDENTITY)
            h[k] = bad
            assert not S.valid(h), (k, bad)


def _edge_vps_of_every_case():
    lines, vps = T.edge_set()
    out = []
    for batch, it in T.edge_cases():
        index = T.indices(it or 0, batch, len(vps), 0, False)
        h = None if it is None else T.augment_transforms(0, it, batch, *T.EDGE_AUGMENT)
        for b, i in enumerate(index):
            if vps[i].shape[0]:
                out.append(vps[i] if h is None else T.transform_vps(h[b], vps[i]))
    return np.concatenate(out, 0)


def test_edge_set_margins():
    """the condition on the inputs of every cell comparison (here and on the GPU): no fractional index within 1e-6 of a
    k + 0.5, for EVERY VP of every case; and the set has the three special images"""
    lines, vps = T.edge_set()
    assert tuple(a.shape[0] for a in lines) == T.EDGE_LINES and tuple(a.shape[0] for a in vps) == T.EDGE_VPS
    allv = _edge_vps_of_every_case()
    for grid in T.EDGE_GRIDS:
        assert T.margin(allv, grid) >= T.MARGIN, grid
    c = T.cells(vps[3], (20, 20))
    assert c[0] == c[1] >= 0                                        # two VPs in one cell
    assert vps[4][0, 2] < 0 and T.cells(vps[4][:1], (20, 20))[0] >= 0
    assert not vps[6][1].any() and T.cells(vps[6], (20, 20))[1] == -1


def test_cells_equal_label_maps():
    allv = _edge_vps_of_every_case()
    for grid in T.EDGE_GRIDS + ((7, 13), (64, 64)):
        assert T.margin(allv, grid) >= T.MARGIN, grid
        assert np.array_equal(S.cells(allv, grid), T.cells(allv, grid)), grid
    assert len(set(S.cells(allv, (20, 20)).tolist())) > 50           # ... over many cells
    assert (S.cells(allv, (1, 1))[np.linalg.norm(allv, axis=1) > 0] == 0).all()


def test_dropped_vps():
    inside = np.array([-1.0, 0.0, 0.0])                              # alpha = -pi / 2: index -0.5, cell 0
    mirror = (-1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    moved = T.transform_vps(mirror, inside[None])[0]                 # alpha = +pi / 2: index gh - 0.5, one past the map
    v = np.array([[0.0, 0.0, 0.0], [np.nan, 0.1, 1.0], [0.1, np.inf, 1.0], moved, inside, [0.0, 1.0, 0.0]])
    for grid in ((20, 20), (4, 4)):
        want = T.cells(v, grid)
        assert want.tolist()[:4] == [-1, -1, -1, -1] and want[4] >= 0, (grid, want)
        assert np.array_equal(S.cells(v, grid), want), grid
    assert S.cells(v, (20, 20))[5] == -1                             # beta = pi / 2 is one past the map too


def test_slots():
    off = np.array([0, 0, 1, 1, 1, 64, 65, 65, 70], dtype=np.int64)
    want = np.repeat(np.arange(8), np.diff(off))
    assert np.array_equal(S.slots(off), want)
    assert np.array_equal(S.slots(np.array([0, 5])), np.zeros(5))


def test_augment():
    ident = train.Augment().transforms(3, 7, 9)
    assert ident.shape == (9, 6) and np.array_equal(ident, np.tile(np.array(IDENTITY), (9, 1)))
    assert train.Augment().is_identity() and not train.Augment(mirror=0.5).is_identity()
    knobs = (0.3, 1.25, 0.1, 0.5)
    aug = train.Augment(*knobs)
    seen_mirror = set()
    for it in (0, 5, 2 ** 40):
        h = aug.transforms(2, it, 32)
        assert np.array_equal(h, T.augment_transforms(2, it, 32, *knobs))
        det = h[:, 0] * h[:, 4] - h[:, 1] * h[:, 3]
        s = np.sqrt(np.abs(det))
        assert (s >= 1 / 1.25 - 1e-12).all() and (s <= 1.25 + 1e-12).all()
        assert (np.abs(h[:, 2]) <= 0.1).all() and (np.abs(h[:, 5]) <= 0.1).all()
        theta = np.arctan2(h[:, 3] * np.sign(det), h[:, 4])          # h10 = s sin m, h11 = s cos
        assert (np.abs(theta) <= 0.3 + 1e-12).all()
        seen_mirror |= set(np.sign(det).tolist())
        assert all(S.valid(row) for row in h)
    assert seen_mirror == {-1.0, 1.0}
    assert not np.array_equal(aug.transforms(2, 0, 4), aug.transforms(2, 1, 4))
    assert np.array_equal(aug.transforms(2, 5, 32)[:4], aug.transforms(2, 5, 4))     # a slot's draws do not depend on B
    assert (np.sign(train.Augment(mirror=1.0).transforms(0, 0, 8)[:, 0]) == -1).all()
    with pytest.raises(ValueError):
        train.Augment(max_scale=0.5)


class _OrderOnly(train.TrainSet):
    """TrainSet's host side without a device"""

    def __init__(self, n):
        self.n = n
        self._orders = {}


def test_order():
    n = 10
    ts = _OrderOnly(n)
    assert np.array_equal(ts.order(4, 0, False), np.arange(n))
    epochs = [ts.order(4, e, True) for e in range(3)]
    for e, o in enumerate(epochs):
        assert sorted(o.tolist()) == list(range(n))
        assert o.tolist() == T.order(4, e, n, True)
    assert not np.array_equal(epochs[0], epochs[1]) and not np.array_equal(epochs[1], epochs[2])
    assert not np.array_equal(ts.order(5, 0, True), epochs[0])
    # Caffe's cursor
    assert ts.indices(0, 4, 0, False).tolist() == [0, 1, 2, 3]
    assert ts.indices(2, 4, 0, False).tolist() == [8, 9, 0, 1]
    assert ts.indices(3, 32, 0, False).tolist() == [(96 + b) % n for b in range(32)]
    assert ts.indices(2 ** 33, 5, 0, False).tolist() == [(2 ** 33 * 5 + b) % n for b in range(5)]
    # a shuffled batch that crosses the end of epoch 0 continues in epoch 1's order
    got = ts.indices(2, 4, 4, True).tolist()
    assert got == epochs[0][8:].tolist() + epochs[1][:2].tolist()
    assert ts.indices(0, 32, 4, True).tolist() == (epochs[0].tolist() + epochs[1].tolist() + epochs[2].tolist() +
                                                   ts.order(4, 3, True).tolist())[:32]
    for it, b in ((0, 1), (7, 5), (3, 32)):
        assert ts.indices(it, b, 4, True).tolist() == T.indices(it, b, n, 4, True)
        assert ts.indices(it, b, 4, True).dtype == np.int32


class _StubRuntime(object):
    class torch(object):
        @staticmethod
        def stack(items):
            class _Host(object):
                def __init__(self, a):
                    self.a = np.asarray(a, dtype=np.float32)

                def cpu(self):
                    return self

                def numpy(self):
                    return self.a
            return _Host(items)


class _StubTrainer(object):
    def __init__(self):
        self.iteration = 0
        self.rt = _StubRuntime()
        self.calls = []

    def step(self, rasters, labels):
        self.calls.append(("step", self.iteration, rasters))
        self.iteration += 1
        return 0.5, None

    def evaluate(self, rasters, labels):
        self.calls.append(("evaluate", self.iteration, rasters))
        return 0.25, None

    def state(self):
        return {"iteration": self.iteration, "seed": 7, "conv_weights": [np.arange(3, dtype=np.float32)], "conv_momentum": [],
                "head_weights": [], "head_momentum": []}

    def load_state(self, d):
        self.loaded = d
        self.iteration = d["iteration"]


class _StubSet(object):
    def batch(self, iteration, batch, seed=0, augment=None, shuffle=False):
        return ("batch", iteration, batch, seed, shuffle), None


def test_solver_schedule(tmp_path):
    want = [("test", 0), ("display", 0), ("display", 2), ("test", 3), ("snapshot", 4), ("display", 4), ("test", 6),
            ("display", 6), ("snapshot", 7)]                         # written by hand from Caffe's Solver::Step and Solve
    assert T.schedule(7, 3, 2, 4) == want
    lines = []
    tr = _StubTrainer()
    prefix = str(tmp_path / "stub")
    sv = train.Solver(tr, _StubSet(), test_set=_StubSet(), batch_size=3, test_batch=2, test_iter=2, test_interval=3, display=2,
                      snapshot=4, snapshot_prefix=prefix, max_iter=7, shuffle=True, seed=11, log=lines.append)
    assert sv.solve() == 7 and tr.iteration == 7
    assert sv.history == want
    assert sorted(os.listdir(str(tmp_path))) == ["stub_iter_4.solverstate.npz", "stub_iter_7.solverstate.npz"]
    steps = [c for c in tr.calls if c[0] == "step"]
    assert [c[1] for c in steps] == list(range(7))
    assert all(c[2] == ("batch", c[1], 3, 11, True) for c in steps)                  # the batch of iteration t
    tests = [c for c in tr.calls if c[0] == "evaluate"]
    assert [c[1] for c in tests] == [0, 0, 3, 3, 6, 6]
    assert [c[2] for c in tests[:2]] == [("batch", 0, 2, 0, False), ("batch", 1, 2, 0, False)]   # the cursor from 0, identity
    assert len(lines) == 7 and lines[0].startswith("Iteration 0, Testing net") and lines[1] == "Iteration 0, loss = 0.5"
    # a multiple of test_interval at the end tests once more; no prefix: no snapshot; no test set: no test
    tr2 = _StubTrainer()
    sv2 = train.Solver(tr2, _StubSet(), test_set=_StubSet(), test_iter=1, test_interval=3, display=0, snapshot=4, max_iter=6,
                       log=None)
    sv2.solve()
    assert sv2.history == [("test", 0), ("test", 3), ("test", 6)] == [e for e in T.schedule(6, 3, 0, 4) if e[0] == "test"]
    tr3 = _StubTrainer()
    sv3 = train.Solver(tr3, _StubSet(), display=0, max_iter=3, log=None)
    sv3.solve()
    assert sv3.history == [] and tr3.iteration == 3
    with pytest.raises(ValueError):
        sv3.snapshot()
    with pytest.raises(ValueError):
        sv3.test()
    # restore: the trainer's state and the data seed
    tr4 = _StubTrainer()
    sv4 = train.Solver(tr4, _StubSet(), seed=99, log=None)
    saved = sv4.restore(prefix + "_iter_4.solverstate.npz")
    assert tr4.iteration == 4 and tr4.loaded["seed"] == 7 and sv4.seed == 11 and saved["batch_size"] == 3
    assert np.array_equal(tr4.loaded["conv_weights"][0], np.arange(3, dtype=np.float32)) and tr4.loaded["head_weights"] == []
    assert sv4.step(2) is not None and tr4.iteration == 6 and tr4.calls[0][2] == ("batch", 4, 5, 11, False)


def test_solver_defaults_match_the_prototxts():
    s = json.load(open(os.path.join(GOLDEN, "train", "solver_settings.json")))
    sig = inspect.signature(train.Solver.__init__).parameters
    for name in ("max_iter", "test_iter", "test_interval", "display", "snapshot"):
        assert sig[name].default == s["solver"][name], name
    assert sig["batch_size"].default == s["batch_size"]["train"] and sig["test_batch"].default == s["batch_size"]["test"]
    assert sig["augment"].default is None and sig["shuffle"].default is False
    sig = inspect.signature(train.TrainSet.__init__).parameters
    assert sig["size"].default == 500 and sig["grid"].default == (20, 20) and sig["alpha"].default == 0.1


def test_abi_names():
    for name in ("vpk_trainset_batch", "vpk_trainset_accumulate"):
        assert name in _lib.EXPORTS
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "vpk.h")).read()
    for name in ("vpk_trainset_batch", "vpk_trainset_accumulate"):
        at = header.index("int " + name + "(")
        assert "train_val.prototxt:1-62" in header[header.rfind("/*", 0, at):at], name
    assert train.MAX_MEAN_IMAGES == (2 ** 32 - 1) // 255 == 16843009
    for cls in (train.NetTrainer, train.StackTrainer):
        assert hasattr(cls, "state") and hasattr(cls, "load_state")
