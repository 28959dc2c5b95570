"""The GPU sphere rasteriser's ORCHESTRATION at its edges (csrc/vpk_raster.hip: what is around the arithmetic that
tests/test_hostsim_raster.py pins on the host): the chunk loop with its per-chunk image order, line base and counters; the
cached offsets; lines with more than one sub-path; outlines around the LDS vertex copy's size; canvas sizes off the
kernels' granules; the blender's table / arithmetic switch; the blend's prefetch clamp between short images; and the C
entry's refusals.  tests/test_gpu_raster.py holds the product paths to the REFERENCE's rasters; here every expected
raster comes from oracle/agg_raster.py (pinned to matplotlib's own output) at run time.

Bar: integer work -- np.array_equal / torch.equal, no tolerance.  The host build of the product arithmetic agrees with the
oracle bit for bit on every input used here (tests/test_hostsim_raster.py), so a mismatch here is the kernels' doing."""
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

inf = np.inf
VPK_ERR_ARG, VPK_ERR_LIMIT = -1, -5                       # include/vpk.h

# a cycle of distinct line sets with 0, 1, 2, 3, 4, 5, 12 and 25 lines: slices of one synthetic scene's lines whose curves
# cross (asserted: every set of two or more piles up above a single line's peak, so the order of the blend matters)
CYCLE = [(0, 0), (0, 1), (1, 3), (3, 6), (6, 10), (10, 15), (15, 27), (15, 40)]
# lines whose samples are finite / NaN in turns (see test_broken_paths): [0], [1] finite, NaN, finite in the default curve;
# [2] NaN then finite, [3] finite then NaN; [4], [5] nothing finite; [6], [7] two finite runs in the `alternative` curve
BROKEN = np.array([[1.5e308, inf, 1.5e308], [1.5e308, -inf, -1.5e308], [inf, 1, inf], [inf, 1, -inf], [0, 0, 0], [np.nan, 1, 1],
                   [1.5e308, 1.5e308, inf], [1.5e308, -1.5e308, -inf]])
TWO_RUNS = {False: (0, 1), True: (6, 7)}                  # curve mode -> the BROKEN lines with two finite runs in it
# lines whose outline polygon at 1024 px has 254 / 256 / 258 / 260 vertices (coverage_kernel keeps up to LVERT = 256 in LDS)
LVERT_LINES = {254: [-2.034167273443428, -0.44257966769355733, 0.7095799877420675],
               256: [1.5906402313231438, -0.17420516361429333, 0.354531946286926],
               258: [-0.1828389745977349, 0.21511530247326374, 1.9350880340988528],
               260: [0.8825389674564839, 0.10688503033029921, 0.09151670328235219]}

_cache = {}


def scene_lines():
    from vanishing_points_2017_amd import synth
    if "a" not in _cache:
        _cache["a"] = synth.make_scene(77, 40, 3, raster=None)["l"]
        _cache["a"].setflags(write=False)
    return _cache["a"]


def want(lines, size, alpha=0.1, alternative=False):
    """The oracle's raster, computed once per input and shared (read-only)."""
    from oracle import agg_raster
    lines = np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 3)
    key = (lines.tobytes(), size, alpha, alternative)
    if key not in _cache:
        with np.errstate(all="ignore"):
            _cache[key] = agg_raster.raster(lines, size=size, alpha=alpha, alternative=alternative)
        _cache[key].setflags(write=False)
    return _cache[key]


def fresh_runtime():
    from vanishing_points_2017_amd.runtime import Runtime
    return Runtime(0)


def release(rt):
    """Give the handle's workspace (gigabytes after a chunked batch) back."""
    rt.synchronize()
    rt.handle.close()
    rt.h = None


def chunks_of(offsets, max_lines):
    """vpk_sphere_raster's chunk rule restated: whole images while offsets[b1 + 1] - offsets[b0] <= max_lines, one image
    at least.  -> [(b0, b1)]"""
    out, b0, batch = [], 0, len(offsets) - 1
    while b0 < batch:
        b1 = b0 + 1
        while b1 < batch and offsets[b1 + 1] - offsets[b0] <= max_lines:
            b1 += 1
        out.append((b0, b1))
        b0 = b1
    return out


def cycle_batch(max_lines):
    """The cycle repeated until the batch is two cycles past max_lines.  -> lines (N x 3), offsets (B + 1), cycles"""
    a = scene_lines()
    per = sum(hi - lo for lo, hi in CYCLE)
    cycles = max_lines // per + 2
    one = np.concatenate([a[lo:hi] for lo, hi in CYCLE])
    counts = np.tile([hi - lo for lo, hi in CYCLE], cycles)
    offsets = np.zeros(counts.size + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    return np.ascontiguousarray(np.tile(one, (cycles, 1))), offsets, cycles


def check_second_chunk(offsets, max_lines):
    """Two chunks; the second starts inside a cycle and holds two different sets at least and an empty image.
    -> (first image of chunk 2, lines in chunk 1, lines in chunk 2)"""
    ch = chunks_of(offsets, max_lines)
    assert len(ch) == 2, ch
    (_, b1), (c0, c1) = ch
    assert b1 == c0 and c0 % len(CYCLE) != 0, c0
    sets = {b % len(CYCLE) for b in range(c0, c1)}
    assert len(sets) >= 2 and 0 in sets, sets
    assert offsets[c0] <= max_lines < offsets[c0 + 1]                 # (the image that did not fit opens chunk 2)
    return c0, int(offsets[c0]), int(offsets[c1] - offsets[c0])


def run_device(rt, l_dev, offsets, size, alpha=0.1, alternative=False, out=None):
    """One raster call on rt's handle in the given curve mode -> device tensor (B, size, size); the flags must be zero."""
    from vanishing_points_2017_amd import sphere_mapping
    rt.check(rt.lib.vpk_sphere_raster_set_alternative(rt.h, 1 if alternative else 0))
    try:
        got = sphere_mapping.raster_batch_device(rt, l_dev, offsets, size, alpha, out=out)
    finally:
        rt.check(rt.lib.vpk_sphere_raster_set_alternative(rt.h, 0))
    rt.synchronize()
    flags = sphere_mapping.raster_flags(rt, len(offsets) - 1)
    assert not flags.any(), np.nonzero(flags)[0][:10]
    return got


def assert_cycle_equals_oracle(rt, got, cycles, size, alternative, what):
    """Every image of the batch == its set's oracle raster: compared on the device, per distinct set over all its
    occurrences."""
    a = scene_lines()
    t = rt.torch
    wants = [want(a[lo:hi], size, 0.1, alternative) for lo, hi in CYCLE]
    for (lo, hi), w in zip(CYCLE, wants):                             # (the premise: a lone line peaks at 25, crossing lines above)
        assert (w.max() > 25) if hi - lo >= 2 else (w.max() == (25 if hi > lo else 0)), (lo, hi, w.max())
    with rt.on_stream():
        exp = t.from_numpy(np.stack(wants)).to(rt.tdev)
        bad = (got.view(cycles, len(CYCLE), size * size) != exp.view(1, len(CYCLE), size * size)).any(dim=2)
        bad = bad.cpu().numpy()                                       # [cycle][set]: this image differs
    for k, (lo, hi) in enumerate(CYCLE):
        assert not bad[:, k].any(), "%s: the %d-line set differs from the oracle in %d of %d images, first at image %d" % (
            what, hi - lo, bad[:, k].sum(), cycles, np.nonzero(bad[:, k])[0][0] * len(CYCLE) + k)


def test_chunked_batch_default_mode():
    """A batch a little over the chunk limit of 49 152 lines: the second chunk runs with first_image, line0 > 0, its own
    image order (longest first, stable) and freshly reset queue / bump counters.  7 576 images at 64 px."""
    rt = fresh_runtime()
    try:
        lines, offsets, cycles = cycle_batch(49152)
        c0, n1, n2 = check_second_chunk(offsets, 49152)
        assert (c0, n1, n2) == (7565, 49150, 94)                      # (what the rule gives for this cycle; for the record)
        with rt.on_stream():
            l_dev = rt.torch.from_numpy(lines).to(rt.tdev)
        got = run_device(rt, l_dev, offsets, 64)
        assert_cycle_equals_oracle(rt, got, cycles, 64, False, "default mode")
    finally:
        release(rt)


def test_chunked_batch_alternative_mode_and_the_mode_switch_on_one_handle():
    """At 500 px the `alternative` curve's chunk limit is min(49152, 3 GiB / (size (size + 2))) = 12 833 lines: a batch a
    little over it is two chunks in that mode and one in the default mode.  Same list, one handle, default -> alternative
    -> default: a stale image order table after a switch would mix images."""
    rt = fresh_runtime()
    try:
        size = 500
        max_alt = min(49152, (3 << 30) // (size * (size + 2)))
        assert max_alt == 12833
        lines, offsets, cycles = cycle_batch(max_alt)
        c0, n1, n2 = check_second_chunk(offsets, max_alt)
        assert (c0, n1, n2) == (1975, 12819, 77)
        assert len(chunks_of(offsets, 49152)) == 1
        with rt.on_stream():
            l_dev = rt.torch.from_numpy(lines).to(rt.tdev)
        for alternative in (False, True, False):
            got = run_device(rt, l_dev, offsets, size, alternative=alternative)
            assert_cycle_equals_oracle(rt, got, cycles, size, alternative, "alternative=%s" % alternative)
            del got
    finally:
        release(rt)


def test_same_offsets_other_lines():
    """Two consecutive calls with identical offsets: the second uploads nothing and waits for nothing.  Each result is
    its own lines' raster, and the second call leaves the first call's output alone."""
    from vanishing_points_2017_amd import sphere_mapping
    rt = fresh_runtime()
    try:
        a = scene_lines()
        first, second = [a[:5], a[:0], a[5:9]], [a[20:25], a[:0], a[30:34]]
        offsets = np.array([0, 5, 5, 9], dtype=np.int64)
        t = rt.torch
        with rt.on_stream():
            l1 = t.from_numpy(np.concatenate(first)).to(rt.tdev)
            l2 = t.from_numpy(np.concatenate(second)).to(rt.tdev)
            out1 = t.full((3, 64, 64), 7, dtype=t.uint8, device=rt.tdev)
            out2 = t.full((3, 64, 64), 9, dtype=t.uint8, device=rt.tdev)
        sphere_mapping.raster_batch_device(rt, l1, offsets, 64, 0.1, out=out1)
        rt.synchronize()
        got1 = out1.cpu().numpy()
        sphere_mapping.raster_batch_device(rt, l2, offsets.copy(), 64, 0.1, out=out2)     # (another host array, same values)
        rt.synchronize()
        assert not sphere_mapping.raster_flags(rt, 3).any()
        got2 = out2.cpu().numpy()
        for lines, r in zip(first, got1):
            assert np.array_equal(r, want(lines, 64))
        for lines, r in zip(second, got2):
            assert np.array_equal(r, want(lines, 64))
        assert not np.array_equal(got1, got2)
        assert np.array_equal(out1.cpu().numpy(), got1)
    finally:
        release(rt)


def broken_mix():
    a = scene_lines()
    return np.concatenate([a[:6], BROKEN[:1], a[6:9], BROKEN[1:], a[9:12]])


def finite_runs(line, size, alternative):
    from oracle import agg_raster
    with np.errstate(all="ignore"):
        x, y = agg_raster.curve_pixels(np.asarray(line, dtype=np.float64), size, alternative=alternative)
    idx = np.nonzero(np.isfinite(x) & np.isfinite(y))[0]
    return 0 if idx.size == 0 else 1 + int((np.diff(idx) > 1).sum())


@pytest.mark.parametrize("alternative", [False, True])
@pytest.mark.parametrize("size", [500, 64])
def test_broken_paths(size, alternative, monkeypatch):
    """Lines with more than one sub-path (finite, NaN, finite samples: the `more` bits of the dense table, its q >= 1
    entries, the blend's inner loop), with a NaN half before or after the finite one (the wave kernel's hand-off to the
    sequential machine) and with nothing to draw, between ordinary crossing lines of one image; that image between an
    ordinary one and an empty one.  Also with every line through the sequential machine: the same bytes."""
    from vanishing_points_2017_amd import sphere_mapping
    from vanishing_points_2017_amd.runtime import get_runtime
    a = scene_lines()
    mix = broken_mix()
    for k in TWO_RUNS[alternative]:
        assert finite_runs(BROKEN[k], size, alternative) == 2, k
    assert finite_runs(BROKEN[2], size, False) == 1 and finite_runs(BROKEN[3], size, False) == 1
    assert finite_runs(BROKEN[4], size, alternative) == 0 and finite_runs(BROKEN[5], size, alternative) == 0
    assert (want(mix, size, 0.1, alternative) != want(a[:12], size, 0.1, alternative)).sum() > 100   # (the broken lines ARE drawn)
    sets = [a[12:20], mix, a[:0]]
    fast = sphere_mapping.raster_batch(sets, size=size, alpha=0.1, alternative=alternative)
    assert not sphere_mapping.raster_flags(get_runtime(0), len(sets)).any()
    for k, (lines, r) in enumerate(zip(sets, fast)):
        assert np.array_equal(r, want(lines, size, 0.1, alternative)), "image %d: %d pixels differ" % (
            k, (r != want(lines, size, 0.1, alternative)).sum())
    monkeypatch.setenv("VPK_RASTER_SEQUENTIAL", "1")
    slow = sphere_mapping.raster_batch(sets, size=size, alpha=0.1, alternative=alternative)
    monkeypatch.delenv("VPK_RASTER_SEQUENTIAL")
    assert not sphere_mapping.raster_flags(get_runtime(0), len(sets)).any()
    assert np.array_equal(fast, slow), "%d pixels differ" % (fast != slow).sum()


def test_outlines_around_the_lds_vertex_copy():
    """Polygons of 254, 256 (the copy's last slot: vert[256] = vert[0]), 258 and 260 vertices (read from HBM, with the
    wrap at the polygon's end) at 1024 px, in one image between ordinary lines and as images of their own.  Each of them
    covers more pixels than coverage_kernel's LDS pool holds at this size: several row bands per polygon."""
    from oracle import agg_raster
    from vanishing_points_2017_amd import sphere_mapping
    from vanishing_points_2017_amd.runtime import get_runtime
    size = 1024
    rowcap = (size + 63) & ~63
    pool = ((53 - 11) * 1024 - 6 * rowcap * 4) // 8 & ~63             # vpk_sphere_raster: COV_LDS, COV_STATIC, six row arrays
    assert pool == 2304
    for n, line in LVERT_LINES.items():
        line = np.array(line)
        assert len(agg_raster.stroke_outline(agg_raster.simplify(*agg_raster.curve_pixels(line, size)), 100 / 72)) == n
        assert len(agg_raster.line_coverage(line, size)) > pool
    a = scene_lines()
    four = np.array([LVERT_LINES[n] for n in (254, 256, 258, 260)])
    together = np.concatenate([a[:4], four[:2], a[4:6], four[2:], a[6:8]])
    sets = [together] + [four[k:k + 1] for k in range(4)]
    got = sphere_mapping.raster_batch(sets, size=size, alpha=0.1)
    assert not sphere_mapping.raster_flags(get_runtime(0), len(sets)).any()
    for k, (lines, r) in enumerate(zip(sets, got)):
        assert np.array_equal(r, want(lines, size)), "image %d: %d pixels differ" % (k, (r != want(lines, size)).sum())
    alone = sphere_mapping.raster_batch([together], size=size, alpha=0.1)[0]
    assert np.array_equal(alone, want(together, size))


@pytest.mark.parametrize("size,alpha", [(8, 0.1), (9, 0.1), (33, 0.1), (65, 0.1), (1023, 0.1), (1024, 0.1), (1024, 0.3)])
def test_canvas_sizes_off_the_granules(size, alpha):
    """The minimum and the maximum size and sizes that are no multiple of the pixel rows' padding (4), the column segments
    (4), the blend's 32 rows per workgroup or the row arrays' 64.  Below 32 px most column segments own no pixel."""
    from vanishing_points_2017_amd import sphere_mapping
    from vanishing_points_2017_amd.runtime import get_runtime
    a = scene_lines()
    got = sphere_mapping.raster_batch([a[:10]], size=size, alpha=alpha)
    assert got.shape == (1, size, size)
    assert not sphere_mapping.raster_flags(get_runtime(0), 1).any()
    exp = want(a[:10], size, alpha)
    assert exp.max() > 0
    assert np.array_equal(got[0], exp), "%d pixels differ" % (got[0] != exp).sum()


def test_the_blenders_table_switch_and_its_extremes():
    """Colour alphas up to BLEND_LUT_MAX_A8 = 63 blend through the LDS tables, larger ones through the arithmetic: both
    sides of the switch, the one-row table of alpha 0 (nothing is drawn), the smallest alpha and saturation at 1."""
    from vanishing_points_2017_amd import sphere_mapping
    a = scene_lines()
    alphas = [0.0, 0.002, 0.247, 0.25, 1.0]
    assert [int(al * 255 + 0.5) for al in alphas] == [0, 1, 63, 64, 255]
    got = {}
    for al in alphas:
        got[al] = sphere_mapping.raster_batch([a[:20]], size=64, alpha=al)[0]
        exp = want(a[:20], 64, al)
        assert np.array_equal(got[al], exp), "alpha %r: %d pixels differ" % (al, (got[al] != exp).sum())
    assert not got[0.0].any()
    assert not np.array_equal(got[0.247], got[0.25])
    assert got[1.0].max() == 255


def test_sphere_line_plot_scales_the_callers_lines_in_place():
    """sphere_line_plot(lines, size, f=2): columns 0 and 1 of the caller's array are scaled in place, as the reference
    does (sphere_mapping.py:55-56), and the raster is the scaled lines'."""
    from vanishing_points_2017_amd import sphere_mapping
    a = scene_lines()
    lines = a[:10].copy()
    got = sphere_mapping.sphere_line_plot(lines, 500, f=2.0)
    scaled = a[:10] * np.array([2.0, 2.0, 1.0])
    assert np.array_equal(lines, scaled)
    assert np.array_equal(got, want(scaled, 500))
    assert not np.array_equal(got, want(a[:10], 500))


def test_refusals_of_the_c_entry():
    """vpk_sphere_raster called directly with what it must refuse: VPK_ERR_ARG for a bad argument, VPK_ERR_LIMIT -- before
    anything is allocated -- for an image whose coverage pool would reach 4 GiB, the message naming the largest line count
    that passes.  After every refusal the handle rasterises an ordinary batch correctly."""
    from vanishing_points_2017_amd import _lib, sphere_mapping
    rt = fresh_runtime()
    try:
        t = rt.torch
        a = scene_lines()
        sets = [a[:5], a[5:9]]
        with rt.on_stream():
            l_dev = t.from_numpy(np.concatenate(sets)).to(rt.tdev)
            out = t.zeros((3, 64, 64), dtype=t.uint8, device=rt.tdev)
        good = np.array([0, 5, 9], dtype=np.int64)

        def call(l, offsets, batch, size, alpha, o):
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            with rt.on_stream():
                return rt.lib.vpk_sphere_raster(rt.h, rt.ptr(l), offsets.ctypes.data_as(ctypes.c_void_p), batch, size, alpha,
                                                rt.ptr(o))

        def still_works():
            got = sphere_mapping.raster_batch(sets, size=64, alpha=0.1, runtime=rt)
            for lines, r in zip(sets, got):
                assert np.array_equal(r, want(lines, 64))
            assert not sphere_mapping.raster_flags(rt, 2).any()

        still_works()
        nan = float("nan")
        bad = {"size 7": (l_dev, good, 2, 7, 0.1), "size 1025": (l_dev, good, 2, 1025, 0.1),
               "alpha -0.1": (l_dev, good, 2, 64, -0.1), "alpha 1.1": (l_dev, good, 2, 64, 1.1), "alpha NaN": (l_dev, good, 2, 64, nan),
               "batch 0": (l_dev, good, 0, 64, 0.1), "offsets not monotone": (l_dev, [0, 6, 5, 9], 3, 64, 0.1),
               "l NULL with lines": (None, good, 2, 64, 0.1)}
        for what, (l, offsets, batch, size, alpha) in bad.items():
            assert call(l, offsets, batch, size, alpha, out) == VPK_ERR_ARG, what
            assert "vpk_sphere_raster" in rt.lib.vpk_last_error(rt.h).decode(), what
            still_works()
        with pytest.raises(_lib.VpkError):
            sphere_mapping.raster_flags(rt, 3)                        # (another batch than the last call's)
        still_works()

        def accepted(lines, size, per_line):                          # the entry's condition restated: the pool stays below 4 GiB
            return max((lines + 4) * per_line, 8 * size * (size + 2)) < 1 << 32

        # (the refusing side only: one line fewer would allocate many GB)
        for alternative, size, lines, per_line in ((False, 8, 262140, 16384), (True, 1024, 4085, 1024 * 1026)):
            assert accepted(lines - 1, size, per_line) and not accepted(lines, size, per_line)
            with rt.on_stream():
                many = t.zeros((lines, 3), dtype=t.float64, device=rt.tdev)
                o = t.zeros((1, size, size), dtype=t.uint8, device=rt.tdev)
            rt.check(rt.lib.vpk_sphere_raster_set_alternative(rt.h, 1 if alternative else 0))
            try:
                rc = call(many, [0, lines], 1, size, 0.1, o)
            finally:
                rt.check(rt.lib.vpk_sphere_raster_set_alternative(rt.h, 0))
            msg = rt.lib.vpk_last_error(rt.h).decode()
            assert rc == VPK_ERR_LIMIT, (rc, msg)
            m = re.search(r"more than (\d+) lines", msg)
            assert m and int(m.group(1)) == lines - 1, msg
            still_works()
    finally:
        release(rt)
