"""The dense head's training step without a GPU: the host build of csrc/train_device.hpp's per-element functions
(tests/hostsim/sim_train.cpp) against the float64 reference (tests/train_reference.py), the dropout mask hash, label_maps,
the solver's defaults against the reference prototxts' numbers (tests/golden/train/solver_settings.json) and the C-ABI."""
import json
import os
import re

import numpy as np
import pytest

import train_reference as R
from conftest import GOLDEN, ROOT
from hostsim import simlib_train
from vanishing_points_2017_amd import coordinate_conversion as cc

ZS = [0.0, 1e-8, -1e-8, 20.0, -20.0, 90.0, -90.0, 700.0, -700.0]
TS = [0.0, 0.3, 1.0]


def _ulp32(x):
    """the spacing of float32 at |x| (at least the smallest subnormal)"""
    x = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def test_loss_and_gradient_at_the_edges():
    """finite and within 2 ulp of float32 of the float64 value on the same float32 inputs, saturated logits included"""
    z = np.array([a for a in ZS for _ in TS], dtype=np.float32)
    t = np.array([b for _ in ZS for b in TS], dtype=np.float32)
    inv_b = np.float32(0.25)                                     # B = 4: exact, so that the bound is on the function alone
    loss, sig, grad = simlib_train.loss(z, t, inv_b)
    z64, t64 = z.astype(np.float64), t.astype(np.float64)
    want_loss = R.loss_terms(z64, t64)
    want_sig = R.sigmoid(z64)
    e = np.exp(-np.abs(z64))                                     # (sigmoid - t) / B without cancellation in the reference
    want_grad = np.where(z64 >= 0, (1 - t64) - t64 * e, e * (1 - t64) - t64) / (1 + e) * float(inv_b)
    for name, got, want in (("loss", loss, want_loss), ("sigmoid", sig, want_sig), ("gradient", grad, want_grad)):
        assert np.isfinite(got).all(), name
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= 2 * _ulp32(want)).all(), (name, z[np.argmax(err / _ulp32(want))], t[np.argmax(err / _ulp32(want))])
    assert np.abs(want_grad - (want_sig - t64) * float(inv_b)).max() <= 1e-16      # it IS (sigmoid - t) / B


def test_learning_rate_policy():
    p = R.DEFAULTS
    want = {0: 1e-4, 199999: 1e-4, 200000: 1e-5, 400000: 1e-6}
    for it, lr in want.items():
        got = simlib_train.learning_rate(p["base_lr"], p["gamma"], p["stepsize"], it)
        assert got == R.learning_rate32(p, it), it                                   # the float32 product chain, to the bit
        assert abs(float(got) - lr) <= 3 * 2.0 ** -24 * lr, (it, got)              # two roundings of the inputs, <= 2 products


def test_sgd_update_of_one_element():
    rs = np.random.RandomState(5)
    w, v, g = (rs.standard_normal(64).astype(np.float32) * s for s in (1.0, 1e-3, 0.1))
    lr_w, de_w, lr_b, de_b, mu, _ = R.local_rates(R.DEFAULTS, 200000)
    for lr, de in ((lr_w, de_w), (lr_b, de_b)):
        wn, vn = simlib_train.sgd_update(w, v, g, lr, de, mu)
        w64, v64, g64 = (a.astype(np.float64) for a in (w, v, g))
        wr, vr, ew, ev = R._update(w64, v64, g64, np.zeros(64), lr, de, mu, True)
        assert np.abs(vr).min() > 0 and not np.array_equal(vn, v)
        assert (np.abs(vn - vr) <= ev).all() and (np.abs(wn - wr) <= ew).all()
        assert (ev <= 4 * 2.0 ** -24 * np.abs(vr) + 1e-12).all()                     # the bound itself is a few ulp
    assert de_b == 0.0 and lr_b == 2 * lr_w


def test_mask_hash():
    b, h = 32, 4096
    m = simlib_train.mask(7, 3, 6, b, h)
    assert m.dtype == np.uint8 and set(np.unique(m)) == {0, 1}
    assert np.array_equal(m, simlib_train.mask(7, 3, 6, b, h))                       # the same key: the same bits
    n = b * h
    assert abs(m.mean() - 0.5) <= 5 * 0.5 / np.sqrt(n)                               # keep fraction within 5 sigma
    # a unit's bit does not depend on how many units or rows are generated with it (no launch geometry in the key)
    assert np.array_equal(simlib_train.mask(7, 3, 6, 5, 100), m[:5, :100])
    # the integer restatement of the documented hash
    for bb, j in ((0, 0), (3, 17), (31, 4095)):
        assert m[bb, j] == R.mask_bit(7, 3, 6, bb, j)
    seen = [m]
    for seed, it, layer in ((7, 3, 7), (7, 4, 6), (7, 4, 7), (8, 3, 6), (7, 0, 6), (7, 200000, 6)):
        other = simlib_train.mask(seed, it, layer, b, h)
        assert abs(other.mean() - 0.5) <= 5 * 0.5 / np.sqrt(n)
        for prev in seen:
            assert not np.array_equal(other, prev), (seed, it, layer)
            assert abs((other == prev).mean() - 0.5) <= 5 * 0.5 / np.sqrt(n)         # and no two are correlated
        seen.append(other)
    assert simlib_train.mask(1, 0, 6, 4, 64, dropout_ratio=0.0).all()


def test_label_maps():
    from vanishing_points_2017_amd.train import label_maps
    shape = (20, 20)
    rs = np.random.RandomState(11)
    half = 0.5 * np.pi / 20
    angles = (rs.random_sample((200, 2)) - 0.5) * (np.pi - 1e-9)
    for k, ang in enumerate(angles):
        point = cc.angle_to_point(ang) * (1.0 if k % 2 else -3.0)                   # any length, either sign
        for arg in (ang[None], point[None], point):
            lab = label_maps(arg, shape)
            assert lab.dtype == np.float32 and lab.shape == shape and lab.sum() == 1.0
            cell = np.argwhere(lab == 1.0)[0]
            assert np.abs(cc.index_to_angle(cell, shape) - ang).max() <= half + 1e-9, (k, ang, cell)
    assert label_maps(np.array([[np.pi / 2 + 0.2, 0.0]]), shape).sum() == 0         # outside the map: all zero
    assert label_maps(np.array([[0.0, -np.pi / 2 - 0.1]]), shape).sum() == 0
    assert label_maps(np.zeros((0, 3)), shape).sum() == 0
    two = label_maps(np.array([[0.01, 0.02], [0.02, 0.01], [1.0, -1.0]]), shape)    # two VPs in one cell: a single 1
    assert two.sum() == 2.0 and set(np.unique(two)) == {0.0, 1.0}
    assert label_maps(angles[:3], (10, 40)).shape == (10, 40)


def test_defaults_are_the_prototxts():
    from vanishing_points_2017_amd import _lib
    from vanishing_points_2017_amd.train import SolverParams
    s = json.load(open(os.path.join(GOLDEN, "train", "solver_settings.json")))
    sol, head = s["solver"], s["head"]
    want = {"base_lr": sol["base_lr"], "gamma": sol["gamma"], "stepsize": sol["stepsize"], "momentum": sol["momentum"],
            "weight_decay": sol["weight_decay"]}
    for layer in ("fc6", "fc7", "fc8_20x20"):                                       # one set of multipliers for the head
        assert head[layer]["lr_mult"] == head["fc6"]["lr_mult"] and head[layer]["decay_mult"] == head["fc6"]["decay_mult"]
    want.update(lr_mult_weight=head["fc6"]["lr_mult"][0], lr_mult_bias=head["fc6"]["lr_mult"][1],
                decay_mult_weight=head["fc6"]["decay_mult"][0], decay_mult_bias=head["fc6"]["decay_mult"][1])
    assert s["dropout_ratio"]["drop6"] == s["dropout_ratio"]["drop7"]
    want["dropout_ratio"] = s["dropout_ratio"]["drop6"]
    assert sol["type"] == "SGD" and sol["lr_policy"] == "step"
    assert SolverParams().as_dict() == want
    assert {k: v for k, v in R.DEFAULTS.items()} == want
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("libvpk.so not built (run python -m vanishing_points_2017_amd.build)")
    got = SolverParams.library_defaults().as_dict()                                 # vpk_train_default_params, as float32
    assert got == {k: (float(np.float32(v)) if k != "stepsize" else v) for k, v in want.items()}
    # the synthetic weights' biases are the prototxt's fillers
    from vanishing_points_2017_amd import cnn
    assert [head[k]["num_output"] for k in ("fc6", "fc7", "fc8_20x20")] == [sh[0] for _, sh in cnn.LAYER_SHAPES[5:]]


def test_abi_names():
    from vanishing_points_2017_amd import _lib
    names = ["vpk_train_create", "vpk_train_destroy", "vpk_train_default_params", "vpk_train_set_params", "vpk_train_load",
             "vpk_train_store", "vpk_train_set_iteration", "vpk_train_get_iteration", "vpk_train_step", "vpk_train_eval",
             "vpk_train_load_momentum", "vpk_train_store_momentum"]
    for n in names:
        assert n in _lib.EXPORTS, n
    header = open(os.path.join(ROOT, "include", "vpk.h")).read()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header), n
    assert "vpk_train.hip" in __import__("vanishing_points_2017_amd.build", fromlist=["UNITS"]).UNITS
