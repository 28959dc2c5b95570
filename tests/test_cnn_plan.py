"""The forward plan of the CNN (csrc/cnn_plan.hpp: cnn_resolve_plan) against the rules as include/vpk.h words them.

The C++ resolver is compiled with g++ (tests/hostsim/sim_cnn_plan.cpp: no HIP) and asked for every combination of
vpk_cnn_set_precision 0..3 x vpk_cnn_set_algorithm 0..4 x vpk_cnn_set_fusion 0..4 x tap in {none, 0..10} x {uint8, float images} x
{device-counted pass, ordinary}: 4 800 plans.  `expected` below restates, stage by stage, what vpk.h documents for those setters
(and for vpk_cnn_forward_f32 / vpk_cnn_set_range_policy); it shares no code and no structure with the resolver."""
import ctypes
import itertools

import pytest

from hostsim import hostbuild


# the enums of cnn_plan.hpp, in declaration order
C1_GEMM, C1_DIRECT_F32, C1_GEMM_FUSED, C1_PIECES3, C1_PIECES2 = range(5)
DMA_F32, SPLIT_GEMM, WINOGRAD, PIECES3, PIECES2 = range(5)
D_DMA_F32, D_PIECES3, D_PIECES2_STREAMED, D_PIECES2_PRESPLIT = range(4)

MSG_COUNTED = "run_forward: a device-counted pass runs algorithm 2 with the default conv1, untapped"
MSG_FUSION4 = "vpk_cnn_forward_f32: vpk_cnn_set_fusion(4) takes uint8 rasters only"


@pytest.fixture(scope="module")
def sim():
    lib = hostbuild.load("cnn_plan")
    lib.sim_cnn_plan.argtypes = [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_int), ctypes.c_char_p]
    lib.sim_cnn_plan.restype = None
    return lib


def resolve(lib, precision, algorithm, fusion, tap, f32, counted, presplit=1, profiling=0):
    out = (ctypes.c_int * 33)()
    msg = ctypes.create_string_buffer(128)
    lib.sim_cnn_plan(precision, algorithm, fusion, presplit, profiling, tap, int(f32), int(counted), out, msg)
    plan = {"err": out[0], "msg": msg.value.decode(), "prep_input": bool(out[1]), "conv1": out[2],
            "conv1_hands_planes": bool(out[3]), "norm2_planes": bool(out[4]), "norm2_hands_planes": bool(out[5]),
            "fc": [out[6], out[7], out[8]], "conv": []}
    for i in range(4):
        o = out[9 + 6 * i: 15 + 6 * i]
        plan["conv"].append({"impl": o[0], "split_tiling": o[1], "chained_in": bool(o[2]), "chained_out": bool(o[3]),
                             "needs_to_planes": bool(o[4]), "writes_next_planes": bool(o[5])})
    return plan


def expected(precision, algorithm, fusion, tap, f32, counted, presplit=1, profiling=0):
    """vpk.h, stage by stage.  Taps: 0 conv1, 1 pool1, 2 conv2, 3 pool2, 4 conv3, 5 conv4, 6 conv5, 7 pool5, 8 fc6, 9 fc7, 10 fc8."""
    # vpk_cnn_set_range_policy: the recompute pass is "the vpk_cnn_set_algorithm(2) forward with the default conv1" -- and nothing else
    if counted and not (precision == 0 and algorithm == 2 and fusion == 3 and tap == -1 and not profiling):
        return {"err": "state", "msg": MSG_COUNTED}
    # vpk_cnn_set_fusion: "0 separate conv1 and LRN / pooling kernels (also used whenever tap 0 is requested)"
    if fusion == 0 or tap == 0:
        conv1 = C1_GEMM
    elif fusion == 1:
        conv1 = C1_DIRECT_F32
    elif fusion == 2:
        conv1 = C1_GEMM_FUSED
    elif fusion == 3:
        conv1 = C1_PIECES3
    else:
        conv1 = C1_PIECES2
    # vpk_cnn_forward_f32: "every arithmetic mode accepts it except vpk_cnn_set_fusion(4) (VPK_ERR_STATE: its fp16 conv1 needs
    # integer pixels)" -- the fp16 conv1, i.e. not when the separate kernels run in its place
    if f32 and conv1 == C1_PIECES2:
        return {"err": "state", "msg": MSG_FUSION4}
    e = {"err": 0, "msg": "", "conv1": conv1}
    # the implicit-GEMM forms of conv1 read f32 phase planes, the direct kernels read the rasters themselves
    e["prep_input"] = conv1 in (C1_GEMM, C1_GEMM_FUSED)

    # vpk_cnn_set_precision(1..3): conv2..5 as three bf16 pieces in the implicit GEMM; vpk_cnn_set_algorithm is "(precision 0)"
    split = precision >= 1
    pairs = not split and algorithm == 4          # "4 (default) DIRECT convolutions (and fc6's weight stream) ... SCALED PAIR of fp16"

    def conv_impl(n):                             # n = 2 .. 5
        if split:
            return SPLIT_GEMM
        if algorithm == 4:
            return PIECES2
        if algorithm == 0:                        # "0 direct: implicit GEMM over the taps"
            return DMA_F32
        if algorithm == 1:                        # "1 Winograd's minimal filtering ... conv2 by F(2 x 2, 5 x 5), conv3..conv5 by F(2 x 2, 3 x 3)"
            return WINOGRAD
        if algorithm == 2:                        # "2 conv2 ... and fc6 on the bf16 matrix cores with EXACT operands; conv3..conv5 as in 1"
            return PIECES3 if n == 2 else WINOGRAD
        return PIECES3 if n in (2, 3, 5) else WINOGRAD   # "3 (measurements) conv2, conv3 and conv5 as in 2's conv2, conv4 as in 1"

    impl = {n: conv_impl(n) for n in (2, 3, 4, 5)}
    # Who hands piece planes to conv n, and the tap of the f32 blob that hand-over skips.  Only the fp16-pair kernels write planes
    # (conv1's fused piece kernel, the pair norm2 / pool2, conv3 and conv4 on pairs); a tapped blob is always written as f32 and
    # converted for the next layer.
    e["norm2_planes"] = pairs
    producer_writes_planes = {2: pairs and conv1 in (C1_PIECES3, C1_PIECES2), 3: pairs, 4: pairs, 5: pairs}
    blob_tap = {2: 1, 3: 3, 4: 4, 5: 5}
    handed = {n: producer_writes_planes[n] and tap != blob_tap[n] for n in (2, 3, 4, 5)}
    e["conv1_hands_planes"] = handed[2]
    e["norm2_hands_planes"] = handed[3]
    # split GEMM: conv3 -> conv4 -> conv5 pass the split format on unless a caller taps conv3 or conv4
    chain = split and tap not in (4, 5)
    # vpk_cnn_set_precision 2, 3 (development): one tiling for every layer; 1: conv2 / conv3 on two 4-wave workgroups per CU
    tiling = {n: (1 if n <= 3 else 0) if precision == 1 else precision - 2 for n in (2, 3, 4, 5)}
    e["conv"] = []
    for n in (2, 3, 4, 5):
        on_pieces = impl[n] in (PIECES3, PIECES2)
        e["conv"].append({
            "impl": impl[n],
            "split_tiling": tiling[n] if split else None,
            "chained_in": chain and n in (4, 5),
            "chained_out": chain and n in (3, 4),
            "needs_to_planes": on_pieces and not handed[n],
            "writes_next_planes": n in (3, 4) and handed[n + 1],
        })
    # fc6 with conv2's arithmetic; the activation scales name fc7's input too: fc7 runs on pairs; fc8 always on the f32 GEMM
    pair_dense = D_PIECES2_PRESPLIT if presplit else D_PIECES2_STREAMED
    if pairs:
        e["fc"] = [pair_dense, pair_dense, D_DMA_F32]
    elif not split and algorithm in (2, 3):
        e["fc"] = [D_PIECES3, D_DMA_F32, D_DMA_F32]
    else:
        e["fc"] = [D_DMA_F32] * 3
    return e


def check(lib, err_state, *args, **kw):
    got, want = resolve(lib, *args, **kw), expected(*args, **kw)
    where = "precision %d algorithm %d fusion %d tap %d f32 %d counted %d %r" % (args + (kw,))
    if want["err"] == "state":
        assert got["err"] == err_state and got["msg"] == want["msg"], where
        return False
    assert got["err"] == 0 and got["msg"] == "", where
    for k in ("prep_input", "conv1", "conv1_hands_planes", "norm2_planes", "norm2_hands_planes", "fc"):
        assert got[k] == want[k], (where, k, got[k], want[k])
    for i in range(4):
        for k, v in want["conv"][i].items():
            if v is not None:
                assert got["conv"][i][k] == v, (where, "conv%d" % (i + 2), k, got["conv"][i][k], v)
    return True


def all_combinations():
    return itertools.product(range(4), range(5), range(5), range(-1, 11), (False, True), (False, True))


def test_every_combination_resolves_to_the_documented_plan(sim):
    err_state = sim.sim_vpk_err_state()
    assert err_state == -4
    n = accepted = 0
    for args in all_combinations():
        n += 1
        accepted += check(sim, err_state, *args)
    assert n == 4800
    # ordinary passes: everything but float images into the fp16 conv1 (4 x 5 x 11 taps: tap 0 runs the separate kernels);
    # device-counted: one configuration, for either image type
    assert accepted == 2400 - 4 * 5 * 11 + 2


def test_prep_input_runs_exactly_for_the_gemm_forms_of_conv1(sim):
    for args in all_combinations():
        precision, algorithm, fusion, tap, f32, counted = args
        plan = resolve(sim, *args)
        if plan["err"] == 0:
            assert plan["prep_input"] == (tap == 0 or fusion in (0, 2)), args
            assert (plan["conv1"] == C1_GEMM) == (tap == 0 or fusion == 0), args


def test_a_tapped_blob_is_written_as_f32(sim):
    # the producer of a tapped blob hands nothing over, and a piece consumer converts the f32 blob itself
    consumer_of = {1: 0, 3: 1, 4: 2, 5: 3}           # tap -> index of the conv stage that reads the blob
    for args in all_combinations():
        tap = args[3]
        plan = resolve(sim, *args)
        if plan["err"] or tap not in consumer_of:
            continue
        handed = {1: plan["conv1_hands_planes"], 3: plan["norm2_hands_planes"], 4: plan["conv"][1]["writes_next_planes"],
                  5: plan["conv"][2]["writes_next_planes"]}[tap]
        assert not handed, args
        c = plan["conv"][consumer_of[tap]]
        assert not c["chained_in"], args
        if c["impl"] in (PIECES3, PIECES2):
            assert c["needs_to_planes"], args


def test_float_images_into_the_fp16_conv1_are_refused_unless_the_gemm_form_runs(sim):
    err_state = sim.sim_vpk_err_state()
    for precision, algorithm, tap in itertools.product(range(4), range(5), range(-1, 11)):
        plan = resolve(sim, precision, algorithm, 4, tap, True, False)
        if tap == 0:
            assert plan["err"] == 0 and plan["conv1"] == C1_GEMM
        else:
            assert plan["err"] == err_state and plan["msg"] == MSG_FUSION4
        assert resolve(sim, precision, algorithm, 4, tap, False, False)["err"] == 0


def test_a_device_counted_pass_is_the_exact_configuration_only(sim):
    err_state = sim.sim_vpk_err_state()
    ok = 0
    for args in all_combinations():
        if not args[5]:
            continue
        for profiling in (0, 1):
            plan = resolve(sim, *args, profiling=profiling)
            if args[:4] == (0, 2, 3, -1) and not profiling:
                assert plan["err"] == 0, args
                assert plan["conv1"] == C1_PIECES3 and [c["impl"] for c in plan["conv"]] == [PIECES3, WINOGRAD, WINOGRAD, WINOGRAD]
                assert not plan["norm2_planes"] and plan["fc"] == [D_PIECES3, D_DMA_F32, D_DMA_F32]
                ok += 1
            else:
                assert plan["err"] == err_state and plan["msg"] == MSG_COUNTED, args
    assert ok == 2


def test_the_dense_presplit_knob_only_picks_the_pair_stream(sim):
    for args in all_combinations():
        a, b = resolve(sim, *args, presplit=1), resolve(sim, *args, presplit=0)
        if a["err"]:
            assert b["err"] == a["err"]
            continue
        assert [D_PIECES2_STREAMED if x == D_PIECES2_PRESPLIT else x for x in a["fc"]] == b["fc"], args
        assert check(sim, -4, *args, presplit=0)
