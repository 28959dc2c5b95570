"""Float images through the CNN (include/vpk.h: vpk_cnn_forward_f32 / vpk_cnn_forward_tap_f32; cnn.image_kind).

The reference writes `image - mean` into Caffe's float32 data blob (evaluation.py:34-38), so any real-valued 500 x 500 image is a
valid input.  A float image must be used as its float32 rounding -- never truncated to uint8 -- under every arithmetic mode, with
the accuracy rule of the uint8 path (factor 1 against the f32 direct kernels, measured against the float64 net on the SAME float
input), the same bits as the uint8 raster when its values are the integers 0..255, and the range flags and policy of the uint8
path.  Synthetic weights and mean."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H_MAX = 65504.0
MARGIN = 1.1
INPUT_TAPS = (1, 3, 4, 5, 7, 8)          # the inputs of conv2, conv3, conv4, conv5, fc6, fc7


def _rasters(n, start=10):
    from vanishing_points_2017_amd import sphere_mapping, synth
    return sphere_mapping.raster_batch([s["l"] for s in synth.config_scenes(2, count=n, start=start)])


def _blur(x):
    """Separable Gaussian blur (sigma 1, 5 taps, edges clamped) of each image of a (B, 500, 500) batch, in float64."""
    k = np.exp(-0.5 * np.arange(-2, 3) ** 2)
    k /= k.sum()
    x = np.asarray(x, np.float64)
    for ax in (1, 2):
        p = np.pad(x, [(0, 0)] + [(2, 2) if a == ax else (0, 0) for a in (1, 2)], mode="edge")
        x = sum(k[i] * np.take(p, np.arange(i, i + 500), axis=ax) for i in range(5))
    return x


def _float_images(n, start=10):
    """n non-integer float32 images, cycling through four kinds: a raster x 0.5 + 0.25, a blurred raster, a raster scaled to
    [0, 1] and uniform noise in [0, 255)."""
    r = _rasters(n, start).astype(np.float64)
    rng = np.random.default_rng(start)
    out = np.empty((n, 500, 500), np.float32)
    for i in range(n):
        kind = i % 4
        if kind == 0:
            out[i] = r[i] * 0.5 + 0.25
        elif kind == 1:
            out[i] = _blur(r[i:i + 1])[0]
        elif kind == 2:
            out[i] = r[i] / 255.0
        else:
            out[i] = rng.uniform(0.0, 255.0, (500, 500))
    return out


@pytest.fixture(scope="module")
def model():
    from vanishing_points_2017_amd import cnn
    w, mean = cnn.synthetic_weights(0), cnn.synthetic_mean(0)
    return w, mean, cnn.Net(w, mean)


def test_float_images_meet_the_factor_1_rule(model):
    """Against the float64 net on the float32 image, the defaults (fusion 3, algorithm 4) and algorithm 2 are no further than the
    f32 direct kernels (fusion 1, algorithm 0) on the same float input, plus 6e-8 of the blob's scale, at pool1, conv2, pool2,
    conv3, conv4, conv5, fc6 and the output.  (Truncating the images to uint8 fails this by orders of magnitude.)  B = 3 and 7,
    and a batch of [0, 1] images alone."""
    from oracle import cnn_torch
    w, mean, net = model
    report = {}
    batches = {"3": _float_images(3), "7": _float_images(7, start=40), "unit": _float_images(10, start=70)[2::4]}
    try:
        for label, x in batches.items():
            ref, taps = cnn_torch.forward(w, mean, x, want_taps=True, dtype=np.float64)
            for tap in (1, 2, 3, 4, 5, 6, 8):                      # pool1, conv2, pool2, conv3, conv4, conv5, fc6
                want = taps[cnn_torch.TAPS[tap]]
                scale = float(np.abs(want).max())
                err = {}
                for name, (fusion, algorithm) in (("direct_f32", (1, 0)), ("default", (3, 4)), ("triples", (3, 2))):
                    net.set_fusion(fusion)
                    net.set_algorithm(algorithm)
                    out, got = net.forward(x, tap=tap)
                    err[name] = (float(np.abs(got.reshape(want.shape) - want).max()), float(np.abs(out - ref).max()))
                report[(label, cnn_torch.TAPS[tap])] = (err, scale)
                for name in ("default", "triples"):
                    assert err[name][0] <= err["direct_f32"][0] + 6e-8 * scale, (name, label, cnn_torch.TAPS[tap], err, scale)
                    assert err[name][1] <= err["direct_f32"][1] + 6e-8, (name, label, cnn_torch.TAPS[tap], err)
                    assert err[name][1] <= 2e-5
    finally:
        net.set_fusion(3)
        net.set_algorithm(4)
    print({k: {n: round(e[0] / v[1], 9) for n, e in v[0].items()} for k, v in report.items()})


def test_integer_valued_float_images_give_the_uint8_bits(model):
    """float32 and float64 images whose values are the integers 0..255 give the uint8 rasters' bits through Net.forward,
    caffe_forward and forward_device, at B = 3, 102 and 4097 (two chunks: device tensors only)."""
    import torch
    from vanishing_points_2017_amd import cnn
    _, _, net = model
    r102 = _rasters(102)
    for batch in (3, 102):
        r = r102[:batch]
        want = net.forward(r)
        for dt in (np.float32, np.float64):
            assert np.array_equal(net.forward(r.astype(dt)), want), (batch, dt)
    for i in range(3):
        want = cnn.caffe_forward(net, r102[i])
        for dt in (np.float32, np.float64):
            assert np.array_equal(cnn.caffe_forward(net, r102[i].astype(dt)), want), (i, dt)
    rt = net.rt

    def on_device(x):
        out = net.forward_device(x)
        rt.synchronize()                  # (the forward runs on the handle's stream)
        return out.cpu().numpy()

    for batch in (3, 102, 4097):
        d8 = torch.from_numpy(np.resize(r102, (batch, 500, 500))).to(rt.tdev)
        want = on_device(d8)
        for dt in (torch.float32, torch.float64):
            got = on_device(d8.to(dt))
            assert np.array_equal(got, want), (batch, dt)
        del d8
        torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", ["algorithm0", "algorithm1", "algorithm2", "algorithm3", "algorithm4", "precision1",
                                  "fusion0", "fusion1", "fusion2"])
def test_every_mode_accepts_float_images(model, mode):
    """Every arithmetic mode runs float images (the f32 pre-pass for the unfused paths, the float loaders of the fused conv1
    kernels) within 2e-5 of the float32 oracle on a non-integer batch."""
    from oracle import cnn_torch
    w, mean, net = model
    x = _float_images(5, start=90)
    ref = cnn_torch.forward(w, mean, x)
    kind, value = mode[:-1], int(mode[-1])
    try:
        getattr(net, "set_" + kind)(value)
        got = net.forward(x)
    finally:
        net.set_fusion(3)
        net.set_algorithm(4)
        net.set_precision(0)
    assert np.abs(got - ref).max() <= 2e-5, (mode, float(np.abs(got - ref).max()))


def test_fusion_4_refuses_float_images(model):
    """The scaled fp16-pair conv1 (vpk_cnn_set_fusion(4)) needs integer pixels: a float forward is an error, never a map."""
    from vanishing_points_2017_amd._lib import VpkError
    _, _, net = model
    x = _float_images(2, start=5)
    try:
        net.set_fusion(4)
        with pytest.raises(VpkError):
            net.forward(x)
    finally:
        net.set_fusion(3)
    assert np.isfinite(net.forward(x)).all()


def test_float_forward_is_bit_reproducible(model):
    """The same float batch twice, and on a fresh Net of the same weights, gives the same bits (B = 7 and 102)."""
    from vanishing_points_2017_amd import cnn
    w, mean, net = model
    fresh = cnn.Net(w, mean)
    for batch in (7, 102):
        x = _float_images(batch, start=200)
        a = net.forward(x)
        assert np.array_equal(net.forward(x), a), batch
        assert np.array_equal(fresh.forward(x), a), batch


def _hot_layer(maxima, target):
    """(layer, e) with maxima[target, layer] * 2^e >= MARGIN x 65 504 and every other image's <= 65 504 / MARGIN, or None."""
    for li in range(maxima.shape[1]):
        for e in range(-40, 80):
            v = maxima[:, li] * 2.0 ** e
            hot, cold = v >= MARGIN * H_MAX, v <= H_MAX / MARGIN
            if (hot | cold).all() and hot[target] and hot.sum() == 1:
                return li, e
    return None


def test_range_flags_and_policy_on_a_float_batch(model):
    """One image of a float batch is scaled up (x 16, a float image can be any size) and one layer's activation scale is raised
    until that image's pairs clamp and no other image's do.  RAISE: VpkRangeError, and image_range_flags names that image.
    RECOMPUTE_EXACT: no error; that image's map is the algorithm-2 float forward of it alone, and every other image's map has the
    bits of the same batch without it."""
    from vanishing_points_2017_amd._lib import VpkRangeError
    _, _, net = model
    x = _float_images(7, start=300)
    target = 3
    x[target] = x[0] * 16.0
    good = net.activation_scales()
    maxima = np.zeros((x.shape[0], 6))
    try:
        net.set_fusion(1)
        net.set_algorithm(0)
        for li, tap in enumerate(INPUT_TAPS):
            _, t = net.forward(x, tap=tap)
            maxima[:, li] = np.abs(t.reshape(x.shape[0], -1)).max(axis=1)
    finally:
        net.set_fusion(3)
        net.set_algorithm(4)
    pick = _hot_layer(maxima, target)
    assert pick is not None, maxima
    li, e = pick
    scales = list(good)
    scales[li] = float(np.ldexp(1.0, int(np.log2(scales[li])) + e))
    rest = np.delete(x, target, axis=0)
    try:
        net.set_algorithm(2)
        alone = net.forward(x[target:target + 1])[0]
        net.set_algorithm(4)
        net.set_activation_scales(scales)
        with pytest.raises(VpkRangeError):
            net.forward(x)
        flags = net.image_range_flags(x.shape[0])
        assert [i for i in range(x.shape[0]) if flags[i]] == [target], flags
        assert flags[target] & (1 << (li + 1)), (flags, li)
        net.set_range_policy("recompute_exact")
        net.recomputed()
        got = net.forward(x)
        assert net.recomputed() == 1
        assert np.array_equal(got[target], alone)
        assert np.array_equal(np.delete(got, target, axis=0), net.forward(rest))
    finally:
        net.set_range_policy("raise")
        net.set_algorithm(4)
        net.set_activation_scales(good)
        net.range_flags()


def test_run_cnn_on_float_and_mixed_pickles(model, tmp_path):
    """evaluation.run_cnn on pickles whose sphere_image is float, and on a mix of uint8 and float pickles (np.stack makes the
    whole batch float): every map equals caffe_forward of its own image, and the uint8 rasters keep their uint8 bits."""
    from vanishing_points_2017_amd import cnn, evaluation
    _, _, net = model
    r = _rasters(4, start=500)
    f = _float_images(4, start=500)
    for name, images in (("float", [f[0], f[1], f[2].astype(np.float64)]), ("mixed", [r[0], f[0], r[1], f[3], r[2]])):
        files = []
        for i, img in enumerate(images):
            p = os.path.join(str(tmp_path), "%s_%d.pkl" % (name, i))
            evaluation._dump_pickle({"lines": None, "sphere_image": img}, p)
            files.append(p)
        evaluation.run_cnn({"pickle_files": files, "destination_folder": str(tmp_path)}, None, None, None, net=net)
        for p, img in zip(files, images):
            pred = evaluation._load_pickle(p)["cnn_prediction"]
            assert pred.shape == (20, 20) and pred.dtype == np.float32
            assert np.array_equal(pred, cnn.caffe_forward(net, img)), (name, p)
            if img.dtype == np.uint8:
                assert np.array_equal(pred, net.forward(img[None])[0]), (name, p)
