"""The CNN's geometry (csrc/cnn_model.hpp) against cnn/deploy.prototxt's arithmetic and the tile shapes of the kernel headers.

The header is compiled with g++ (tests/hostsim/sim_cnn_model.cpp: no HIP) and asked, the way vpk_cnn.hip asks it, for every struct the
kernels take by value -- for every layer, field by field --, the work items of every launch at the batches where a rounding steps, the
im2col tap tables and the arena.  The expected values below are derived here from the net (channels, kernel, stride, padding, groups:
deploy.prototxt) and from the tiles as the kernel headers' comments state them; they share no code with the header."""
import ctypes

import pytest

from hostsim import hostbuild

BATCHES = [1, 4, 5, 102, 128, 129, 257, 4096]       # conv1's groups of 4, 128 / 256 columns, Winograd's 64 and 30 tiles; the largest chunk
INT_MAX = 2 ** 31 - 1

# deploy.prototxt: (input channels, input size, output channels, kernel, stride, pad, groups); LRN + 3 x 3 / 2 max pooling (ceil
# mode) follow conv1 and conv2, the pooling alone conv5
CONV = [(1, 500, 96, 11, 4, 0, 1), (96, 61, 256, 5, 1, 2, 2), (256, 30, 384, 3, 1, 1, 1), (384, 30, 384, 3, 1, 1, 2), (384, 30, 256, 3, 1, 1, 2)]
FC = [(57600, 4096), (4096, 4096), (4096, 400)]
KSPLIT = {5: 72, 6: 16, 7: 32}                       # split-K of the f32 GEMM's dense layers
GEMM_BM = [96, 128, 128, 96, 128, 128, 128, 128]     # cnn_gemm_f32.hpp: conv1 and conv4 (2 x 192 channels) on 96 x 128 tiles, the others 128 x 128


def cdiv(a, b):
    return -(-a // b)


def conv_out(size, k, s, p):
    return (size + 2 * p - k) // s + 1


def pool_out(size):
    return cdiv(size - 3, 2) + 1


def out_border(li):                                  # the border a conv layer's output planes carry: the consumer's padding, if it is a conv
    return CONV[li + 1][5] if li in (2, 3) else 0


def test_the_net_chains():
    assert conv_out(500, 11, 4, 0) == 123 and pool_out(123) == 61 and conv_out(61, 5, 1, 2) == 61 and pool_out(61) == 30
    assert conv_out(30, 3, 1, 1) == 30 and pool_out(30) == 15 and 256 * 15 * 15 == FC[0][0]


@pytest.fixture(scope="module")
def sim():
    lib = hostbuild.load("cnn_model")
    ll, i, f = ctypes.POINTER(ctypes.c_longlong), ctypes.c_int, ctypes.c_float
    dbl = ctypes.POINTER(ctypes.c_double)
    lib.sim_conv_dims.argtypes = [i, i, i, ll]
    lib.sim_split_dims.argtypes = [i, i, ll]
    lib.sim_piece_dims.argtypes = [i, i, i, i, f, f, f, ll, dbl]
    lib.sim_wino_dims.argtypes = [i, i, ll]
    lib.sim_wino5_dims.argtypes = [i, i, ll]
    lib.sim_dense_dims.argtypes = [i, i, i, f, f, ll, dbl]
    lib.sim_total.argtypes = [i, i, i, i]
    lib.sim_total.restype = ctypes.c_longlong
    lib.sim_ew_blocks.argtypes = [ctypes.c_longlong]
    lib.sim_ew_blocks.restype = ctypes.c_longlong
    lib.sim_ktab.argtypes = [i, ctypes.POINTER(ctypes.c_uint), i]
    lib.sim_input_planes.argtypes = [i, ll]
    lib.sim_regions.argtypes = [ll]
    lib.sim_regions.restype = ctypes.c_longlong
    lib.sim_taps.argtypes = [ll]
    return lib


def record(fn, n, *args):
    out = (ctypes.c_longlong * n)()
    fn(*(args + (out,)))
    return list(out)


def named(names, values):
    assert len(names.split()) == len(values)
    return dict(zip(names.split(), values))


# ---- the structs, field by field ------------------------------------------------------------------------------------------------------
CONV_FIELDS = "B IC Hp Wp OC OH OW groups K Kp Mp N ksplit relu OHp OWp opad"


def expected_conv_dims(li, B):
    if li < 5:
        cin, size, cout, k, s, p, g = CONV[li]
        o = conv_out(size, k, s, p)
        e = {"IC": cin // g, "Hp": size + 2 * p, "Wp": size + 2 * p, "OC": cout // g, "OH": o, "OW": o, "groups": g, "K": cin // g * k * k}
        if li == 0:                                  # conv1 reads 4 x 4 stride-4 phase planes of 125 x 125 (prep_input_kernel)
            e.update(IC=16, Hp=125, Wp=125)
    else:
        cin, cout = FC[li - 5]
        e = {"IC": cin, "Hp": 1, "Wp": 1, "OC": cout, "OH": 1, "OW": 1, "groups": 1, "K": cin}
    ob = out_border(li)
    e.update(B=B, Kp=cdiv(e["K"], 16) * 16, Mp=cdiv(e["OC"], GEMM_BM[li]) * GEMM_BM[li], N=B * e["OH"] * e["OW"], ksplit=KSPLIT.get(li, 1),
             relu=1, OHp=e["OH"] + 2 * ob, OWp=e["OW"] + 2 * ob, opad=ob)
    return e


def test_conv_dims_of_every_layer(sim):
    for B in BATCHES:
        for li in range(8):
            got = named(CONV_FIELDS, record(sim.sim_conv_dims, 17, li, B, 0))
            assert got == expected_conv_dims(li, B), (li, B)
            assert got["N"] <= INT_MAX
    got = named(CONV_FIELDS, record(sim.sim_conv_dims, 17, 0, 1, 0))
    assert (got["K"], got["Kp"], got["IC"], got["Hp"], got["Wp"]) == (121, 128, 16, 125, 125)
    assert [named(CONV_FIELDS, record(sim.sim_conv_dims, 17, li, 1, 0))["K"] for li in (1, 2, 3, 4)] == [1200, 2304, 1728, 1728]
    assert [named(CONV_FIELDS, record(sim.sim_conv_dims, 17, li, 1, 0))["ksplit"] for li in (5, 6, 7)] == [72, 16, 32]


def test_conv1_with_the_fused_epilogue(sim):
    # one 128-column tile per patch of 3 x 8 pooled outputs (21 x 8 patches cover 61 x 61), written into pool1's planes: conv2's border of 2
    for B in BATCHES:
        e = expected_conv_dims(0, B)
        e.update(N=B * cdiv(61, 3) * cdiv(61, 8) * 128, OHp=65, OWp=65, opad=2)
        assert named(CONV_FIELDS, record(sim.sim_conv_dims, 17, 0, B, 1)) == e, B


SPLIT_FIELDS = "B Cg Ctot Hp Wp OC OH OW groups KW ntaps csteps ksteps mblocks N relu OHp OWp opad"
SPLIT_BLOCKS = {1: 4, 2: 4, 3: 6, 4: 4}              # 32-row blocks per tile: conv_gemm_split_kernel's WAVES_M x TM = 2 x 2, conv4 2 x 3


def test_split_dims_of_conv2_to_conv5(sim):
    for B in BATCHES:
        for li in range(1, 5):
            cin, size, cout, k, s, p, g = CONV[li]
            ob = out_border(li)
            e = named(SPLIT_FIELDS, [B, cin // g, cin, size + 2 * p, size + 2 * p, cout // g, size, size, g, k, k * k, cin // g // 16,
                                     k * k * (cin // g // 16), cdiv(cdiv(cout // g, 32), SPLIT_BLOCKS[li]) * SPLIT_BLOCKS[li],
                                     B * size * size, 1, size + 2 * ob, size + 2 * ob, ob])
            assert named(SPLIT_FIELDS, record(sim.sim_split_dims, 19, li, B)) == e, (li, B)
    assert [record(sim.sim_split_dims, 19, li, 1)[13] for li in range(1, 5)] == [4, 12, 6, 4]


PIECE_FIELDS = "B Cg16 CGtot Hp Wp OC OH OW groups KW ntaps ksteps mblocks mtiles rtiles ctiles relu OHp OWp opad in_image o_cgtot o_Hp o_Wp o_pad nulls"
# cnn_conv_pieces.hpp: a tile = 128 output channels x 4 rows x 32 columns; conv4 on pairs 64 channels x 8 rows; conv4 on triples 192 channels
PIECE_TILE = {False: {1: (4, 4), 2: (4, 4), 3: (6, 4), 4: (4, 4)}, True: {1: (4, 4), 2: (4, 4), 3: (2, 8), 4: (4, 4)}}   # (32-row blocks, rows)


def piece_dims(sim, li, pairs, B, hand=0, hscale=1.0, ascale=1.0, next_ascale=1.0):
    out = (ctypes.c_longlong * 26)()
    fout = (ctypes.c_double * 2)()
    sim.sim_piece_dims(li, int(pairs), B, hand, hscale, ascale, next_ascale, out, fout)
    return named(PIECE_FIELDS, list(out)), list(fout)


def expected_piece_dims(li, pairs, B):
    cin, size, cout, k, s, p, g = CONV[li]
    blk, rows = PIECE_TILE[pairs][li]
    ob = out_border(li)
    mblocks = cdiv(cdiv(cout // g, 32), blk) * blk
    return named(PIECE_FIELDS, [B, cin // g // 16, cin // 16, size + 2 * p, size + 2 * p, cout // g, size, size, g, k, k * k,
                                k * k * (cin // g // 16), mblocks, mblocks // blk, cdiv(size, rows), cdiv(size, 32), 1, size + 2 * ob,
                                size + 2 * ob, ob,
                                # planes of 16-byte words: [channel group of 16][piece x k half: 2 NP][y][x]
                                (cin // 16) * (4 if pairs else 6) * (size + 2 * p) ** 2 * 16, 0, 0, 0, 0, 1])


def test_piece_dims_of_conv2_to_conv5(sim):
    for B in BATCHES:
        for pairs in (False, True):
            for li in range(1, 5):
                got, (o_ascale, oscale) = piece_dims(sim, li, pairs, B)
                assert got == expected_piece_dims(li, pairs, B), (li, pairs, B)
                assert (o_ascale, oscale) == (0.0, 1.0)
    table = {"mblocks": ([4, 12, 6, 4], [4, 12, 6, 4]), "mtiles": ([1, 3, 1, 1], [1, 3, 3, 1]), "rtiles": ([16, 8, 8, 8], [16, 8, 4, 8]),
             "ctiles": ([2, 1, 1, 1], [2, 1, 1, 1]), "ksteps": ([75, 144, 108, 108], [75, 144, 108, 108])}
    for field, (triples, pairs) in table.items():
        assert [piece_dims(sim, li, False, 1)[0][field] for li in range(1, 5)] == triples, field
        assert [piece_dims(sim, li, True, 1)[0][field] for li in range(1, 5)] == pairs, field


def test_pair_layers_hand_planes_and_scales_on(sim):
    # conv3 -> conv4 -> conv5 on pairs: the epilogue writes the next layer's planes (384 channels = 24 groups, 32 x 32, border 1) with
    # that layer's activation scale, and multiplies by 1 / (weight scale x activation scale)
    for li in (2, 3):
        got, (o_ascale, oscale) = piece_dims(sim, li, True, 5, hand=1, hscale=8192.0, ascale=0.125, next_ascale=0.5)
        e = expected_piece_dims(li, True, 5)
        e.update(o_cgtot=24, o_Hp=32, o_Wp=32, o_pad=1)
        assert got == e and o_ascale == 0.5 and oscale == 1.0 / 1024
    got, (o_ascale, oscale) = piece_dims(sim, 1, False, 5, hscale=8192.0, ascale=0.125)
    assert oscale == 1.0                              # bf16 triples are not scaled


def test_winograd_dims(sim):
    for B in BATCHES:
        for li in (2, 3, 4):                         # F(2 x 2, 3 x 3): 15 x 15 tiles per image, 64 output channels x 8 input channels per stage
            cin, size, cout, k, s, p, g = CONV[li]
            ob = out_border(li)
            assert record(sim.sim_wino_dims, 12, li, B) == [cin // g, cout // g, g, cin, cout, B * 225, cout // g // 64, cin // g // 8,
                                                            size + 2 * ob, size + 2 * ob, ob, 1], (li, B)
        # conv2, F(2 x 2, 5 x 5): 31 x 31 tiles per image (61 x 61 outputs), 64 output channels x 4 input channels
        assert record(sim.sim_wino5_dims, 9, 1, B) == [48, 128, 2, 96, 256, B * 961, 2, 12, 1], B


def dense_dims(sim, li, B, pairs, hscale=1.0, ascale=1.0):
    out = (ctypes.c_longlong * 9)()
    fout = (ctypes.c_double * 2)()
    sim.sim_dense_dims(li, B, int(pairs), hscale, ascale, out, fout)
    return list(out), list(fout)


def test_dense_dims_of_fc6_and_fc7(sim):
    # cnn_dense_pieces.hpp: tiles of 256 outputs x 128 images, chunks of 32 k; fc6 1800 chunks in 45 parts of 40, fc7 128 in 16 parts of 8
    for B in BATCHES:
        assert dense_dims(sim, 5, B, False) == ([B, 57600, 4096, 1800, 45, 40, 16, cdiv(B, 128), 1], [1.0, 1.0])
        assert dense_dims(sim, 6, B, False) == ([B, 4096, 4096, 128, 16, 8, 16, cdiv(B, 128), 1], [1.0, 1.0])
        assert dense_dims(sim, 6, B, True, 16384.0, 0.25) == ([B, 4096, 4096, 128, 16, 8, 16, cdiv(B, 128), 1], [16384.0, 1.0 / 4096])
        assert dense_dims(sim, 5, B, False, 16384.0, 0.25)[1] == [1.0, 1.0]
        # fc6's input fragments, the largest: per 128 images 1800 chunks x (3 pieces x 2 steps x 4 column blocks x 1 KB)
        assert sim.sim_total(12, 0, B, 0) == cdiv(B, 128) * 1800 * 3 * 2 * 4 * 1024


# ---- the work items of every launch ---------------------------------------------------------------------------------------------------
def test_launch_totals(sim):
    seen = 0
    for B in BATCHES:
        want = {}
        for li in range(8):                          # the f32 GEMM: BM x 128 tiles of (channels, positions) x split-K parts
            e = expected_conv_dims(li, B)
            want[(0, li, GEMM_BM[li])] = e["groups"] * e["ksplit"] * cdiv(B * e["OH"] * e["OW"], 128) * cdiv(e["OC"], GEMM_BM[li])
        want[(1, 0, 0)] = B * 21 * 8                 # fused: a tile per patch, all 96 channels
        for group in (1, 3, 4, 64):                  # conv1_pieces_kernel: 168 patch positions x groups of `group` images
            want[(2, 0, group)] = 168 * cdiv(B, group)
        want[(3, 0, 0)] = B * 168                    # conv1_direct_kernel: a patch per work item
        for li in range(1, 5):
            cin, size, cout, k, s, p, g = CONV[li]
            want[(4, li, 0)] = g * cdiv(B * size * size, 256) * cdiv(cdiv(cout // g, 32), SPLIT_BLOCKS[li])
            tiles, per_wg = (B * 961, 30) if li == 1 else (B * 225, 64)
            want[(5, li, 0)] = g * (cout // g // 64) * cdiv(tiles, per_wg)
            for pairs in (False, True):
                blk, rows = PIECE_TILE[pairs][li]
                want[(6, li, int(pairs))] = g * B * cdiv(size, rows) * cdiv(size, 32) * cdiv(cdiv(cout // g, 32), blk)
        want[(7, 5, 0)] = 16 * cdiv(B, 128) * 45
        want[(7, 6, 0)] = 16 * cdiv(B, 128) * 16
        want[(8, 0, 0)] = B * cdiv(96, 16) * cdiv(61, 7) * cdiv(61, 16)      # norm1 + pool1: 16 channels x 7 x 16 pooled outputs
        want[(9, 0, 0)] = B * cdiv(30, 6) * 8        # norm2 + pool2: 6 pooled rows x 8 channel ranges
        want[(10, 0, 0)] = cdiv(B * 256, 8)          # pool5: 8 planes per workgroup
        want[(11, 0, 0)] = B * 256
        for (kind, li, arg), w in want.items():
            got = sim.sim_total(kind, li, B, arg)
            assert got == w, (kind, li, B, arg, got, w)
            assert 0 < got <= INT_MAX
            seen += 1
        # the element-wise grids: 256 threads, one per element -- the split-K reductions, the taps' unpad, conv1's input pass
        for n in [B * 4096, B * 400, B * 96 * 61 * 61, B * 256 * 30 * 30, B * 384 * 30 * 30, 250000, 1, 256, 257]:
            assert sim.sim_ew_blocks(n) == cdiv(n, 256) <= INT_MAX
    assert seen == len(BATCHES) * (8 + 1 + 4 + 1 + 4 * 4 + 2 + 4)
    # the figures of the pieces' table at one image
    assert [sim.sim_total(6, li, 1, 1) for li in range(1, 5)] == [64, 24, 24, 16]
    assert [sim.sim_total(6, li, 1, 0) for li in range(1, 5)] == [64, 24, 16, 16]


# ---- the tap table --------------------------------------------------------------------------------------------------------------------
def test_tap_tables(sim):
    for li in range(5):
        cin, size, cout, k, s, p, g = CONV[li]
        K = cin // g * k * k
        buf = (ctypes.c_uint * 4096)()
        n = sim.sim_ktab(li, buf, 4096)
        assert n == cdiv(K, 16) * 16
        want = []
        for ic in range(cin // g):
            for kh in range(k):
                for kw in range(k):
                    if li == 0:                      # phase plane (kh % 4, kw % 4) of 125 x 125, pixel (kh // 4, kw // 4)
                        want.append(((((kh % 4) * 4 + kw % 4) * 125 + kh // 4) * 125 + kw // 4) * 4)
                    else:                            # plane ic of the bordered input, pixel (kh, kw): bytes from the patch origin
                        want.append(((ic * (size + 2 * p) + kh) * (size + 2 * p) + kw) * 4)
        assert list(buf[:K]) == want, li
        assert list(buf[K:n]) == [0] * (n - K)
    buf = (ctypes.c_uint * 128)()
    assert sim.sim_ktab(0, buf, 128) == 128 and list(buf[121:]) == [0] * 7


# ---- the arena and the taps -----------------------------------------------------------------------------------------------------------
def test_regions_and_taps(sim):
    from vanishing_points_2017_amd import cnn
    out = (ctypes.c_longlong * 32)()
    total = sim.sim_regions(out)
    n = out[0]
    regions = list(out[1:1 + n])
    planes1, planes2, planes34 = 96 * 65 * 65, 256 * 32 * 32, 384 * 32 * 32      # pool1 / pool2 / conv3, conv4 with the consumer's border
    assert regions == [500 * 500, 96 * 123 * 123, planes1, 256 * 61 * 61, planes2, planes34, planes34, 256 * 30 * 30, 256 * 15 * 15,
                       4096, 4096, 72 * 4096,
                       # 16-bit pieces: three per value = 3 / 2 floats
                       planes1 * 3 // 2, planes34 * 3 // 2, planes34 * 3 // 2, planes1 * 3 // 2, planes2 * 3 // 2, planes34 * 3 // 2]
    assert total == sum(regions) == 8079728
    taps = (ctypes.c_longlong * 14)()
    sim.sim_taps(taps)
    want = []
    for shape in cnn.TAP_SHAPES:
        size = 1
        for d in shape:
            size *= d
        want.append(size)
    assert list(taps[:11]) == want
    assert list(taps[11:]) == [250000, 400, 4096]
    # the bordered planes a pooling stage writes and an unpad reads
    assert [record(sim.sim_input_planes, 6, li) for li in (1, 2, 3, 4)] == [[96, 61, 61, 65, 65, 2], [256, 30, 30, 32, 32, 1],
                                                                              [384, 30, 30, 32, 32, 1], [384, 30, 30, 32, 32, 1]]


# ---- the benchmark's roofline counts what the driver launches -------------------------------------------------------------------------
def test_executed_flop_counts_the_launched_work(sim):
    from vanishing_points_2017_amd.cnn import Net
    for fusion in (3, 4):                            # conv1_pieces_kernel: the patches of one image, whatever the group
        tiles = Net.EXEC_CONV1[fusion][0]
        assert tiles == sim.sim_total(2, 0, 1, 1) == sim.sim_total(2, 0, 1, 4)
    assert Net.EXEC_CONV1[1][0] == sim.sim_total(3, 0, 1, 0)
    for li, name in enumerate(("conv2", "conv3", "conv4", "conv5"), start=1):
        tiles, steps = Net.EXEC_PAIRS[name]
        assert tiles == sim.sim_total(6, li, 1, 1), name
        assert steps == piece_dims(sim, li, True, 1)[0]["ksteps"], name
        assert Net.executed_flop(name, algorithm=4) == (tiles * steps * 4 * 12 * 2.0 * 32 * 32 * 16, "f16")
    tiles, steps = Net.EXEC_TRIPLES_CONV2
    assert tiles == sim.sim_total(6, 1, 1, 0) and steps == piece_dims(sim, 1, False, 1)[0]["ksteps"]
    # the returned numbers, as the benchmark has always read them
    assert Net.executed_flop("conv1", fusion=3) == (168 * 12 * 72 * 2.0 * 16 * 16 * 32, "bf16")
    assert Net.executed_flop("conv1", fusion=4) == (168 * 12 * 48 * 2.0 * 16 * 16 * 32, "f16")
    assert Net.executed_flop("conv1", fusion=1) == (168 * 8 * 186 * 2.0 * 16 * 16 * 4, "f32")
    assert Net.executed_flop("conv1", fusion=0) == (2 * 96 * 15129 * 121 * 128.0 / 121.0, "f32")
    assert Net.executed_flop("conv2", algorithm=2) == (64 * 4 * 75 * 24 * 2.0 * 32 * 32 * 16, "bf16")
    assert Net.executed_flop("conv2", algorithm=4) == (64 * 75 * 4 * 12 * 2.0 * 32 * 32 * 16, "f16")
    assert Net.executed_flop("conv4", algorithm=4) == (24 * 108 * 4 * 12 * 2.0 * 32 * 32 * 16, "f16")
