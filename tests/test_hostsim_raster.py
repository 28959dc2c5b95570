"""The rasteriser's PRODUCT code compiled for the host by tests/hostsim/sim_raster.cpp and run by one thread -- the CPU
suite's check of the code the GPU kernels are made of: csrc/raster_curve.hpp (samples, curve, spines, split column),
csrc/raster_device.hpp (simplifier, stroker, cell walker with its clip box and its closed-form restart of AGG's row DDA,
calculate_alpha, blender) and csrc/raster_coverage.hpp (polygon_coverage: the rows' split in a left and a right range, the
rule that joins them, the bands of rows a polygon beyond the cell pool is done in, the sweep's runs, the row table with its
"more sub-paths" bits), at the pool size the product uses and at the smallest one.  What stays with
tests/test_gpu_raster.py and tests/test_gpu_raster_edges.py is what needs the GPU: several threads and their barriers and
atomics, simplify_kernel's wave machine, blend_kernel's fetch pipeline, tables and order across workgroups, the chunk loop
(the latter file's inputs run through the host build at the end of this file).  Bit-exact against the reference's own
rasters (tests/golden) and the restatement oracle/agg_raster.py."""
import functools
import os

import numpy as np
import pytest

from golden_util import load
from hostsim import simlib
from oracle import agg_raster


GOLDENS = ["tiny_n12", "clean3_n60", "noweights_n100", "yud_n330", "stress_n300"]


@functools.lru_cache(maxsize=None)
def golden_raster(name, pool=None):
    """(the golden, the host build's raster of its lines at 500 px, flags, what the coverage path met), computed once"""
    g = load(name)
    return (g,) + simlib.sim_raster(g["l"], 500, 0.1, pool=pool, counters=True)


@pytest.mark.parametrize("name", GOLDENS)
def test_product_arithmetic_reproduces_the_references_raster(name):
    g, got, flags, _ = golden_raster(name)
    assert flags == 0
    diff = got.astype(int) - g["sphere_image"].astype(int)
    assert not diff.any(), "%d pixels differ" % (diff != 0).sum()


def test_the_rows_split_and_join_on_the_way_to_the_references_raster():
    """The pixel equality above could hold with every row one range: on yud_n330 rows keep two separate ranges (the gap
    between them dropped) AND rows are joined (ranges that touch, or a gap that is drawn), both in plenty."""
    g, got, flags, met = golden_raster("yud_n330")
    assert flags == 0 and np.array_equal(got, g["sphere_image"])
    assert met["split_rows"] > 0 and met["joined_rows"] > 0, met


@pytest.mark.parametrize("name", GOLDENS)
def test_polygons_done_in_bands_reproduce_the_references_raster(name):
    """The cell pool at its smallest legal size -- one joined row: size + 2 entries, rounded up to 64 = 512 at 500 px --
    so that polygons take several bands of rows: the same pixels, nothing dropped."""
    g, got, flags, met = golden_raster(name, pool=512)
    assert flags == 0 and met["banded_polygons"] > 0, met
    assert np.array_equal(got, g["sphere_image"])


def test_the_pool_size_of_the_product():
    """A band must hold one joined row (size + 2 entries); the sizes the launch uses today, from its formula: what 53 KB of
    LDS less 11 KB of static arrays and six row arrays (of the size rounded up to 64 ints) leave, in (cover, area) pairs,
    rounded down to 64.  (At 8 px that is 5184 entries: 6 * 64 ints of row arrays.)"""
    for size, pool in ((8, 5184), (500, 3840), (1023, 2304), (1024, 2304)):
        assert pool == ((53 * 1024 - 11 * 1024 - 6 * ((size + 63) & ~63) * 4) // 8) & ~63
        assert simlib.sim_raster_pool(size) == pool >= size + 2
    with pytest.raises(ValueError):                                  # (the host build refuses a smaller pool)
        simlib.sim_raster(np.zeros((0, 3)), 64, 0.1, pool=65)


def test_odd_lines_sizes_and_alpha_against_the_restatement():
    odd = np.array([[1, 0.0, 0.3], [1, 1e-9, 0.3], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.3, -1e-6, -2.0], [1, 1, 1e6],
                    [5, 0.01, 0.01], [0, 0, 1.0]])
    got, flags = simlib.sim_raster(odd, 500, 0.1)
    assert flags == 0 and np.array_equal(got, agg_raster.raster(odd))
    rng = np.random.default_rng(5)
    l = rng.normal(size=(25, 3))
    got, _ = simlib.sim_raster(l, 250, 0.5)
    assert np.array_equal(got, agg_raster.raster(l, size=250, alpha=0.5))
    got, _ = simlib.sim_raster(l[:0], 250, 0.1)                      # no lines: the frame alone
    assert np.array_equal(got, agg_raster.raster(l[:0], size=250))


def test_an_edge_walked_in_shares_gives_the_cells_of_the_edge_walked_whole():
    """coverage_kernel gives the rows of a long edge to up to 32 threads; each restarts AGG's incremental x DDA in closed
    form at its first row.  Same accumulators as the single walk, for edges inside, across and outside the clip box."""
    rng = np.random.default_rng(11)
    size = 64
    n = 0
    for _ in range(400):
        x1, y1, x2, y2 = rng.uniform(-20, size + 20, 4)
        if rng.random() < 0.2:
            x2 = x1 + rng.uniform(-0.3, 0.3)                          # nearly vertical
        if rng.random() < 0.2:
            y2 = y1 + rng.uniform(-0.3, 0.3)                          # within one row
        for k in (2, 5, 32):
            assert simlib.sim_edge_shares(x1, y1, x2, y2, size, k) == 0, (x1, y1, x2, y2, k)
            n += 1
    assert n == 1200


def test_product_arithmetic_on_the_alternative_curve():
    """The `alternative` parametrisation (sphere_mapping.py:58-59) through the product's simplifier / stroker / cells: the
    reference's own rasters (tests/golden/rasteralt.npz), pixel for pixel."""
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "rasteralt.npz"))
    for k in "abc":
        got, flags = simlib.sim_raster(g["l_" + k], 500, 0.1, alternative=True)
        assert flags == 0 and np.array_equal(got, g["raster_" + k]), k


# ---- the inputs of tests/test_gpu_raster_edges.py: "product arithmetic == oracle" on record in the CPU suite, so that a GPU
# ---- mismatch on them points at the kernels' orchestration
@pytest.mark.parametrize("alternative", [False, True])
@pytest.mark.parametrize("size", [500, 64])
def test_broken_paths_against_the_restatement(size, alternative):
    """Lines whose samples are finite / NaN in turns (two sub-paths, a NaN half before or after the finite one, nothing to
    draw) between ordinary crossing lines."""
    from test_gpu_raster_edges import TWO_RUNS, BROKEN, broken_mix, want
    mix = broken_mix()
    for k in TWO_RUNS[alternative]:
        assert len(simlib.sim_outline_counts(BROKEN[k], size, alternative)) == 2, k      # (two polygons in the product too)
    got, flags = simlib.sim_raster(mix, size, 0.1, alternative=alternative)
    assert flags == 0 and np.array_equal(got, want(mix, size, 0.1, alternative))


def test_outlines_around_256_vertices_against_the_restatement():
    """The four 1024-px lines whose outlines have 254 ... 260 vertices: the product's stroker makes polygons of the same
    size as the oracle's (the GPU test picks its lines by that count), and the same pixels."""
    from test_gpu_raster_edges import LVERT_LINES, want
    for n, line in LVERT_LINES.items():
        line = np.array(line)
        assert len(agg_raster.stroke_outline(agg_raster.simplify(*agg_raster.curve_pixels(line, 1024)), 100 / 72)) == n
        assert simlib.sim_outline_counts(line, 1024) == [n]
        got, flags = simlib.sim_raster(line, 1024, 0.1)
        assert flags == 0 and np.array_equal(got, want(line, 1024))
        # ... and with the smallest pool (1024 + 2 entries, rounded up to 64): bands meet the vertices read from beyond LDS
        got, flags, met = simlib.sim_raster(line, 1024, 0.1, pool=1088, counters=True)
        assert flags == 0 and met["banded_polygons"] > 0 and np.array_equal(got, want(line, 1024))


@pytest.mark.parametrize("size", [8, 9, 33])
def test_smallest_canvases_against_the_restatement(size):
    from test_gpu_raster_edges import scene_lines, want
    a = scene_lines()
    got, flags = simlib.sim_raster(a[:10], size, 0.1)
    assert flags == 0 and np.array_equal(got, want(a[:10], size))


@pytest.mark.parametrize("alpha,a8", [(0.0, 0), (0.002, 1), (0.247, 63), (0.25, 64), (1.0, 255)])
def test_alphas_at_the_blenders_edges_against_the_restatement(alpha, a8):
    from test_gpu_raster_edges import scene_lines, want
    assert int(alpha * 255 + 0.5) == a8
    a = scene_lines()
    got, flags = simlib.sim_raster(a[:20], 64, alpha)
    assert flags == 0 and np.array_equal(got, want(a[:20], 64, alpha))
    assert got.max() == {0: 0, 1: 0, 63: 212, 64: 213, 255: 255}[a8]
