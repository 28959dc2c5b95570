"""The rasteriser's PRODUCT arithmetic (csrc/raster_device.hpp: simplifier, stroker, cell walker with its clip box and its
closed-form restart of AGG's row DDA, calculate_alpha, blender) compiled for the host by tests/hostsim/sim_raster.cpp and run
serially -- the CPU suite's check of the code the GPU kernels are made of (the kernels' own orchestration: LDS pools, row
bands, atomics, the blend order across workgroups, is what tests/test_gpu_raster.py and tests/test_gpu_raster_edges.py
cover; the latter's inputs run through the host build at the end of this file).  Bit-exact against the reference's own
rasters (tests/golden) and the restatement oracle/agg_raster.py."""
import os
import sys

import numpy as np
import pytest

from golden_util import load
from oracle import agg_raster

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "hostsim"))
import simlib  # noqa: E402


@pytest.mark.parametrize("name", ["tiny_n12", "clean3_n60", "noweights_n100", "yud_n330", "stress_n300"])
def test_product_arithmetic_reproduces_the_references_raster(name):
    g = load(name)
    got, flags = simlib.sim_raster(g["l"], 500, 0.1)
    assert flags == 0
    diff = got.astype(int) - g["sphere_image"].astype(int)
    assert not diff.any(), "%d pixels differ" % (diff != 0).sum()


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
