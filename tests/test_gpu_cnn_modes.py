"""Every CNN kernel a setter (or a load-time knob) can select, held to the float64 net -- the modes tests/test_gpu_cnn.py does not reach.

tests/test_cnn_plan.py proves on the host that cnn_resolve_plan SELECTS the right kernel for every combination; this module checks on
the GPU that the selected kernels COMPUTE the right thing:

1. accuracy of vpk_cnn_set_fusion(4), vpk_cnn_set_algorithm(3), vpk_cnn_set_precision(2 / 3), VPK_DENSE_PRESPLIT=0 and of
   VPK_CONV1_GROUP other than 4, against oracle.cnn_torch.forward(..., dtype=np.float64) on the same input, beside the f32 direct
   kernels (vpk_cnn_set_fusion(1), vpk_cnn_set_algorithm(0)) on the same input;
2. the production forward (untapped: every hand-off of piece planes / split format active) against the tapped forwards, which write the
   f32 blob and convert it with to_planes_kernel / split_nhwc_kernel: the same split of the same f32 value, so the same bits;
3. tile tails across images (split GEMM: 256 columns, Winograd: 64 / 30 tiles, dense layers: 128 images) in every mode: an image of a
   batch of 129 or 257 carries the bits of its twin in a batch of 5.

The bars are those of tests/test_gpu_cnn.py and DESIGN.md section 3 (scale = max |want| of the tapped float64 blob):
  absolute bar      tap error <= 2e-5 x scale; output error <= 2e-5
  factor-1 rule     (a layer on pieces) tap error <= err(direct f32) + 6e-8 x scale; output error <= err(direct f32) + 6e-8
  split-GEMM rule   tap error <= 3.0 x err(precision 0, algorithm 0) + 1e-7 x scale
  Winograd rule     tap error <= 6.0 x err(direct f32) + 1e-7 x scale
Synthetic weights and mean; the float64 oracle runs (B <= 7) are shared by the module."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABS_BAR = 2e-5
TIE = 6e-8                      # 2^-24 of the blob's scale: ties of the factor-1 rule


def _rasters(n, start):
    from vanishing_points_2017_amd import sphere_mapping, synth
    return sphere_mapping.raster_batch([s["l"] for s in synth.config_scenes(2, count=n, start=start)])


def _restore(net):
    net.set_fusion(3)
    net.set_algorithm(4)
    net.set_precision(0)


def _set(net, fusion, algorithm, precision):
    net.set_fusion(fusion)
    net.set_algorithm(algorithm)
    net.set_precision(precision)


class _Yardstick(object):
    """The inputs of the accuracy tests with their float64 forward, and the errors of the two comparison settings on them -- each
    computed once, when a test first asks."""

    def __init__(self, w, mean, net):
        self.w, self.mean, self.net = w, mean, net
        self._inputs = {}
        self._errors = {}

    def inputs(self, label):
        """(images, float64 response maps, float64 taps) of "3" / "7" (uint8 rasters, B = 3 and an odd B = 7) and "dense" (three
        rasters of >= 800 lines and the all-255 image)."""
        if label not in self._inputs:
            from oracle import cnn_torch
            if label == "dense":
                from test_gpu_cnn import _dense_rasters
                x = _dense_rasters()[0]
            else:
                x = _rasters(int(label), start=10)
            ref, taps = cnn_torch.forward(self.w, self.mean, x, want_taps=True, dtype=np.float64)
            self._inputs[label] = (x, ref, taps)
        return self._inputs[label]

    def measure(self, net, label, tap):
        """(tap error, output error, scale) of `net` as it is set, against the float64 net; tap None: the untapped forward (no tap
        error, scale 1)."""
        from oracle import cnn_torch
        x, ref, taps = self.inputs(label)
        if tap is None:
            out = net.forward(x)
            assert np.isfinite(out).all()
            return 0.0, float(np.abs(out - ref).max()), 1.0
        out, got = net.forward(x, tap=tap)
        assert np.isfinite(out).all() and np.isfinite(got).all()
        want = taps[cnn_torch.TAPS[tap]]
        return float(np.abs(got.reshape(want.shape) - want).max()), float(np.abs(out - ref).max()), float(np.abs(want).max())

    def comparison(self, name, label, tap):
        """The same of "direct_f32" (fusion 1, algorithm 0: one f32 FMA chain per output) or "native" (the default conv1, algorithm 0,
        precision 0: what the split GEMM is measured beside) on the module's net."""
        key = (name, label, tap)
        if key not in self._errors:
            _set(self.net, 1 if name == "direct_f32" else 3, 0, 0)
            try:
                self._errors[key] = self.measure(self.net, label, tap)
            finally:
                _restore(self.net)
        return self._errors[key]


@pytest.fixture(scope="module")
def model():
    from vanishing_points_2017_amd import cnn
    w, mean = cnn.synthetic_weights(0), cnn.synthetic_mean(0)
    net = cnn.Net(w, mean)
    return w, mean, net, _Yardstick(w, mean, net)


@pytest.fixture(scope="module")
def knob_runtime():
    """A handle of this module's own for the nets whose load reads VPK_DENSE_PRESPLIT / VPK_CONV1_GROUP (each load on it replaces
    the previous model): nothing else ever forwards on a net loaded under such a knob."""
    from vanishing_points_2017_amd import runtime
    return runtime.Runtime(0)


def _tap_name(tap):
    from oracle import cnn_torch
    return "output" if tap is None else cnn_torch.TAPS[tap]


def _rel(e):
    return round(e[0] / e[2], 9)


# ---------------------------------------------------------------- 1. modes that nothing measured

@pytest.mark.parametrize("algorithm", [4, 0])
def test_conv1_on_scaled_fp16_pairs_against_the_float64_net(model, algorithm):
    """vpk_cnn_set_fusion(4): conv1_pieces_kernel<2>, the weights as scaled fp16 pairs.  At pool1 (tap 1: what the stage writes) the
    absolute bar and the factor-1 rule against vpk_cnn_set_fusion(1); at the output the factor-1 rule under algorithm 4.  Under
    algorithm 4 the kernel's pooling stage writes conv2's piece planes itself in the untapped forward and under every tap but 1 -- taps
    2 and 3 (conv2, pool2) see what that plane writer handed on --; under algorithm 0 its f32 pool1 blob feeds the f32 kernels.
    B = 3 and an odd B = 7.

    Under algorithm 0 the OUTPUT is held to the absolute bar only, not to factor 1 (include/vpk.h says so under mode 4).  Measured
    on the MI355X at B = 3: pool1 2.4e-7 of its scale against the direct kernel's 5.9e-7 (factor 0.40: the stage itself passes the
    rule), but the output 2.49e-6 against 2.41e-6 (factor 1.034; the default conv1 under algorithm 0: 2.35e-6).  That is the f32 FMA
    chains of conv2 .. fc8 behind it -- ten times conv1's own share -- sampled on a pool1 blob that differs in its last bits: rounding
    alone, no index or hand-off involved (pool1 passes, and under algorithm 4 the output is 0.88e-6 against 2.41e-6).  The ratio is
    printed."""
    _, _, net, ys = model
    report = {}
    try:
        for label in ("3", "7"):
            for tap in ((1, 2, 3, None) if algorithm == 4 else (1, None)):
                want = ys.comparison("direct_f32", label, tap)
                _set(net, 4, algorithm, 0)
                got = ys.measure(net, label, tap)
                scale = got[2]
                report[(label, _tap_name(tap))] = {"direct_f32": (_rel(want), want[1]), "fusion4": (_rel(got), got[1])}
                print((label, _tap_name(tap)), report[(label, _tap_name(tap))])
                assert got[0] <= ABS_BAR * scale, (label, _tap_name(tap), got, want)
                assert got[0] <= want[0] + TIE * scale, (label, _tap_name(tap), got, want)
                assert got[1] <= ABS_BAR
                if algorithm == 4:
                    assert got[1] <= want[1] + TIE, (label, _tap_name(tap), got, want)
                else:
                    print("output error, fusion 4 / fusion 1 under algorithm 0: %.3f" % (got[1] / want[1]))
    finally:
        _restore(net)


def test_conv1_on_scaled_fp16_pairs_on_dense_rasters_and_the_all_255_image(model):
    """vpk_cnn_set_fusion(4) where its operands are largest: rasters of >= 800 lines and the all-255 image (every pixel the largest
    fp16 integer the kernel meets, the accumulators at their largest).  Finite, nothing clamped, the factor-1 rule at pool1 and at
    the output (tapped and untapped, with conv2's planes from the kernel's own writer)."""
    _, _, net, ys = model
    try:
        for tap in (1, None):
            want = ys.comparison("direct_f32", "dense", tap)
            _set(net, 4, 4, 0)
            got = ys.measure(net, "dense", tap)                   # (Net.forward raises VpkRangeError if anything was clamped)
            scale = got[2]
            print(("dense", _tap_name(tap)), {"direct_f32": (_rel(want), want[1]), "fusion4": (_rel(got), got[1])})
            assert got[0] <= ABS_BAR * scale and got[1] <= ABS_BAR, (_tap_name(tap), got, want)
            assert got[0] <= want[0] + TIE * scale, (_tap_name(tap), got, want)
            assert got[1] <= want[1] + TIE, (_tap_name(tap), got, want)
        assert net.range_flags() == 0
    finally:
        _restore(net)


def test_triples_in_conv3_and_conv5_against_the_float64_net(model):
    """vpk_cnn_set_algorithm(3): conv2, conv3, conv5 and fc6 on exact bf16 triples -- conv_pieces_kernel<3, nb, 3, 1> and
    to_planes_kernel<3> at the 3 x 3 layers' shapes, which no other setting runs -- and conv4 by Winograd.  The absolute bar at conv2,
    pool2, conv3, conv4, conv5, fc6 and the output; the factor-1 rule at the layers on triples; conv4 within the Winograd rule."""
    _, _, net, ys = model
    try:
        for label in ("3", "7"):
            for tap in (2, 3, 4, 5, 6, 8, None):
                want = ys.comparison("direct_f32", label, tap)
                _set(net, 3, 3, 0)
                got = ys.measure(net, label, tap)
                scale = got[2]
                print((label, _tap_name(tap)), {"direct_f32": (_rel(want), want[1]), "algorithm3": (_rel(got), got[1])})
                assert got[0] <= ABS_BAR * scale and got[1] <= ABS_BAR, (label, _tap_name(tap), got, want)
                if tap in (2, 4, 6, 8):
                    assert got[0] <= want[0] + TIE * scale, (label, _tap_name(tap), got, want)
                if tap == 5:
                    assert got[0] <= 6.0 * want[0] + 1e-7 * scale, (label, _tap_name(tap), got, want)
    finally:
        _restore(net)


@pytest.mark.parametrize("precision", [2, 3])
def test_forced_split_gemm_tilings_against_the_float64_net(model, precision):
    """vpk_cnn_set_precision(2) / (3): ONE tiling of the split GEMM for conv2, conv3 and conv5 -- 2: the 8-wave workgroup, which
    precision 1 runs for conv5 alone; 3: two 4-wave workgroups, which it runs for conv2 and conv3 alone.  As precision 1 is held in
    test_split_bf16_convolutions_are_as_accurate_as_the_f32_matrix_path: the absolute bar and the split-GEMM rule at conv2, conv3,
    conv4, conv5, fc6 and the output.  Taps 4 and 5 break the conv3 -> conv4 -> conv5 chain (the <.., false> epilogues, f32 blobs
    through split_nhwc_kernel); the untapped forward and taps 2, 6, 8 keep it (the <.., true> epilogues)."""
    _, _, net, ys = model
    try:
        for label in ("3", "7"):
            for tap in (2, 4, 5, 6, 8, None):
                want = ys.comparison("native", label, tap)
                _set(net, 3, 0, precision)
                got = ys.measure(net, label, tap)
                scale = got[2]
                print((precision, label, _tap_name(tap)), {"native": (_rel(want), want[1]), "split": (_rel(got), got[1])})
                assert want[0] <= ABS_BAR * scale and got[0] <= ABS_BAR * scale, (label, _tap_name(tap), got, want)
                assert got[0] <= 3.0 * want[0] + 1e-7 * scale, (label, _tap_name(tap), got, want)
                assert got[1] <= ABS_BAR and want[1] <= ABS_BAR
    finally:
        _restore(net)


def test_dense_layers_on_pairs_split_in_registers(model, knob_runtime, monkeypatch):
    """VPK_DENSE_PRESPLIT=0 (read by vpk_cnn_load): fc6 and fc7 by dense_pieces_kernel<2>, which streams the f32 weights and splits
    them into fp16 pairs in registers, instead of dense_pairs_kernel on the pre-split fragments.  The factor-1 rule at fc6, fc7 and
    the output.  Whether the maps equal the pre-split net's bit for bit is printed, not asserted: the two kernels may sum in another
    order."""
    from vanishing_points_2017_amd import cnn
    w, mean, net, ys = model
    monkeypatch.setenv("VPK_DENSE_PRESPLIT", "0")
    streamed = cnn.Net(w, mean, runtime=knob_runtime)
    monkeypatch.delenv("VPK_DENSE_PRESPLIT")
    for label in ("3", "7"):
        for tap in (8, 9, None):
            want = ys.comparison("direct_f32", label, tap)
            got = ys.measure(streamed, label, tap)
            scale = got[2]
            print((label, _tap_name(tap)), {"direct_f32": (_rel(want), want[1]), "streamed": (_rel(got), got[1])})
            assert got[0] <= ABS_BAR * scale and got[1] <= ABS_BAR, (label, _tap_name(tap), got, want)
            assert got[0] <= want[0] + TIE * scale, (label, _tap_name(tap), got, want)
            assert got[1] <= want[1] + TIE, (label, _tap_name(tap), got, want)
        x = ys.inputs(label)[0]
        a, b = streamed.forward(x), net.forward(x)
        print("B = %s: streamed and pre-split maps bit-equal: %s (max |diff| %.3g)" % (label, np.array_equal(a, b), np.abs(a - b).max()))


@pytest.mark.parametrize("group", [1, 3, 64])
def test_conv1_group_does_not_change_a_bit(model, knob_runtime, monkeypatch, group):
    """VPK_CONV1_GROUP (read by vpk_cnn_load): how many images a work item of conv1_pieces_kernel walks -- never how a pixel is
    computed.  B = 11 ends inside a group of 3 and of 4 and is smaller than 64: pool1 and the response maps must be the bits of the
    default group of 4, for the default conv1 on uint8 rasters and on float images and for vpk_cnn_set_fusion(4) on rasters."""
    from test_gpu_cnn_float_input import _float_images
    from vanishing_points_2017_amd import cnn
    w, mean, net, _ = model
    monkeypatch.setenv("VPK_CONV1_GROUP", str(group))
    other = cnn.Net(w, mean, runtime=knob_runtime)
    monkeypatch.delenv("VPK_CONV1_GROUP")
    rasters = _rasters(11, start=50)
    floats = _float_images(11, start=50)
    assert len({r.tobytes() for r in rasters}) == 11
    try:
        for fusion, x in ((3, rasters), (3, floats), (4, rasters)):
            net.set_fusion(fusion)
            other.set_fusion(fusion)
            want_out, want_pool = net.forward(x, tap=1)
            got_out, got_pool = other.forward(x, tap=1)
            assert np.abs(want_pool).max() > 1.0
            assert np.array_equal(got_pool, want_pool), (group, fusion, x.dtype, np.abs(got_pool - want_pool).max())
            assert np.array_equal(got_out, want_out), (group, fusion, x.dtype)
            assert np.array_equal(other.forward(x), net.forward(x)), (group, fusion, x.dtype)     # conv2's planes from conv1's writer
    finally:
        other.set_fusion(3)
        net.set_fusion(3)


# ---------------------------------------------------------------- 2. the production hand-offs against the tapped conversions

# (fusion, algorithm, precision, accepts float images)
HANDOFF_MODES = {
    "default": (3, 4, 0, True),
    "fusion4": (4, 4, 0, False),
    "precision1": (3, 0, 1, True),
    "precision2": (3, 0, 2, True),
    "precision3": (3, 0, 3, True),
    "algorithm2": (3, 2, 0, True),
    "algorithm3": (3, 3, 0, True),
}
HANDOFF_CASES = [(m, k) for m, v in HANDOFF_MODES.items() for k in (("u8", "f32") if v[3] else ("u8",))]


@pytest.mark.parametrize("mode,kind", HANDOFF_CASES)
def test_tapped_forwards_give_the_bits_of_the_untapped_forward(model, mode, kind):
    """The untapped forward hands piece planes (split format) from a producer's epilogue to the next layer; a forward tapped at t
    writes blob t in f32 and converts it with to_planes_kernel (split_nhwc_kernel).  Both split the same f32 value the same way, so
    the response map of forward(x, tap=t) must be the untapped forward's bit for bit, t = 1 .. 10 -- a hand-off that mislays a border
    row of pieces, or scales differently, differs.  (Tap 0 runs conv1 as the unfused GEMM: another summation order by design.)"""
    from test_gpu_cnn_float_input import _float_images
    _, _, net, _ = model
    fusion, algorithm, precision, _ = HANDOFF_MODES[mode]
    x = _rasters(7, start=10) if kind == "u8" else _float_images(7, start=40)
    try:
        _set(net, fusion, algorithm, precision)
        want = net.forward(x)
        assert np.isfinite(want).all() and np.abs(want - 0.5).max() > 1e-3
        differ = {}
        for tap in range(1, 11):
            out, blob = net.forward(x, tap=tap)
            assert np.isfinite(blob).all()
            if not np.array_equal(out, want):
                differ[_tap_name(tap)] = float(np.abs(out - want).max())
        assert not differ, (mode, kind, differ)
    finally:
        _restore(net)


# ---------------------------------------------------------------- 3. tile tails across images, in every mode

# (fusion, algorithm, precision)
TAIL_MODES = {
    "algorithm0": (3, 0, 0), "algorithm1": (3, 1, 0), "algorithm2": (3, 2, 0), "algorithm3": (3, 3, 0), "algorithm4": (3, 4, 0),
    "precision1": (3, 0, 1), "precision2": (3, 0, 2), "precision3": (3, 0, 3),
    "fusion0": (0, 4, 0), "fusion1": (1, 4, 0), "fusion2": (2, 4, 0), "fusion4": (4, 4, 0),
    "streamed_dense": (3, 4, 0),
}


@pytest.mark.parametrize("mode", list(TAIL_MODES))
def test_batch_composition_does_not_change_a_bit_past_the_tile_boundaries(model, knob_runtime, monkeypatch, mode):
    """Five distinct rasters repeated to B = 129 and B = 257: the split GEMM's 256-column tiles, Winograd's blocks of 64 (conv2: 30)
    tiles and the dense layers' tiles of 128 images then span images and end inside one, and the dense layers run a second column
    tile.  Every image must carry the bits of its twin in the B = 5 forward ("batch composition does not change a result"), in
    every mode."""
    from vanishing_points_2017_amd import cnn
    w, mean, net, _ = model
    if mode == "streamed_dense":
        monkeypatch.setenv("VPK_DENSE_PRESPLIT", "0")
        net = cnn.Net(w, mean, runtime=knob_runtime)
        monkeypatch.delenv("VPK_DENSE_PRESPLIT")
    five = _rasters(5, start=30)
    assert len({r.tobytes() for r in five}) == 5
    try:
        _set(net, *TAIL_MODES[mode])
        small = net.forward(five)
        assert np.isfinite(small).all() and np.abs(small - 0.5).max() > 1e-3
        assert len({m.tobytes() for m in small}) == 5              # (five different maps: a twin is told from its neighbours)
        for batch in (129, 257):
            big = net.forward(np.concatenate([five] * 52)[:batch])
            want = np.concatenate([small] * 52)[:batch]
            wrong = [i for i in range(batch) if not np.array_equal(big[i], want[i])]
            assert not wrong, (mode, batch, len(wrong), wrong[:8], float(np.abs(big - want).max()))
    finally:
        _restore(net)
