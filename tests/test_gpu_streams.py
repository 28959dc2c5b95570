"""Lanes (handle + stream pairs) on one GPU: a second lane and asynchronous batches give the same bits."""
import numpy as np
import pytest

from conftest import golden_cases
from golden_util import load

pytestmark = pytest.mark.gpu


def _scene(g):
    return {"l": g["l"].copy(), "lp": g["lp"], "cnn_response": g["cnn_response"],
            "sphere_image": g["sphere_image"], "init_vp": g.get("init_vp")}


def test_second_lane_matches_default_lane():
    """Two lanes (handle + stream) on one GPU compute the same results; a lane reports the stream it was given."""
    from vanishing_points_2017_amd import cnn, em as gem
    from vanishing_points_2017_amd.runtime import get_runtime
    names = [c for c in golden_cases() if not any(k.startswith("kw_") for k in load(c))][:4]
    gs = [load(n) for n in names]
    rt0 = get_runtime(0)
    rt1 = get_runtime(0, "second")
    assert rt1.handle.lib.vpk_get_stream(rt1.h) == rt1.stream.cuda_stream
    rt1.handle.em_set_workgroups(2)            # four images queue on two workgroups: no result depends on that
    p = gem._params({})
    outs = []
    for rt in (rt0, rt1):
        d = gem.upload_batch(rt, [_scene(g) for g in gs])
        o = gem.em_batch_device(rt, d["offsets"], d["l"], d["lp"], d["cnn"], d["sphere"], None, p)
        rt.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in o.items() if v is not None})
    for k in ("vp", "vp_assoc", "num_vp", "iterations", "sigma"):
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k
    w, mean = cnn.synthetic_weights(0), cnn.synthetic_mean(0)
    x = np.stack([g["sphere_image"] for g in gs])
    y0 = cnn.Net(w, mean, device=0, runtime=rt0).forward(x)
    y1 = cnn.Net(w, mean, device=0, runtime=rt1).forward(x)
    assert np.array_equal(y0, y1)


def test_queued_batches_on_one_lane_are_independent():
    """vpk_em_batch is asynchronous: several batches queued on one stream without host synchronisation
    (the header staging ring wraps) return what they return one at a time."""
    from vanishing_points_2017_amd import em as gem
    from vanishing_points_2017_amd.runtime import get_runtime
    names = [c for c in golden_cases() if not any(k.startswith("kw_") for k in load(c))][:3]
    gs = [load(n) for n in names]
    rt = get_runtime(0)
    p = gem._params({})
    ds = [gem.upload_batch(rt, [_scene(g)]) for g in gs]
    def launch(d, keep):
        with rt.on_stream():           # the copy of l (normalised in place) must be ordered on the lane's stream
            l = d["l"].clone()
        keep.append(l)                 # ... and must outlive the launch that reads it
        return gem.em_batch_device(rt, d["offsets"], l, d["lp"], d["cnn"], d["sphere"], None, p)

    ref, keep = [], []
    for d in ds:
        o = launch(d, keep)
        rt.synchronize()
        ref.append(o["vp"].cpu().numpy())
    outs = []
    for rep in range(3):               # 9 launches back to back: more than the 4 staging buffers
        for d in ds:
            outs.append(launch(d, keep))
    rt.synchronize()
    for k, o in enumerate(outs):
        assert np.array_equal(o["vp"].cpu().numpy(), ref[k % len(ds)], equal_nan=True)


# the batch sizes of nine queued calls.  Ring slot k % 4 stages call k's header: 512 bytes for 1 image (pinned: twice that,
# 1024), 768 for 50 (offsets 51 x 8 -> 512, order 50 x 4 -> 256), 1536 for 97 (98 x 8 -> 1024, 97 x 4 -> 512).
#   alternating: slots 0 and 2 only ever stage the 1-image header, slots 1 and 3 the 97-image header; each is pinned once, the
#                device header is reallocated at call 1 while call 0 is queued, and a reused slot is rewritten with the bytes
#                it held: this sequence covers the wrap and the device header's growth, not a slot's
#   mixed:       every slot is pinned for 1 image first; calls 4 and 7 (slots 0 and 3) free and regrow their slot's pinned
#                buffer while earlier calls are queued, and calls 4, 6, 7 and 8 write a header of another batch into a slot
#                that an earlier call staged: a missing wait for that call's copy would hand it the wrong offsets and order
RING_SEQUENCES = {"alternating": [1, 97, 1, 97, 1, 97, 1, 97, 1], "mixed": [1, 1, 1, 1, 97, 1, 50, 97, 1]}


@pytest.mark.parametrize("name", sorted(RING_SEQUENCES))
def test_ring_wraps_while_the_header_grows(name):
    """Nine vpk_em_batch calls queued on a fresh lane without host synchronisation, with the batch sizes of RING_SEQUENCES: the
    ring of four pinned staging buffers wraps twice while the device header, and in "mixed" a ring slot's pinned buffer, are
    reallocated behind queued calls.  Every call's vp, num_vp, vp_assoc and status equal its batch run alone and synchronised."""
    from vanishing_points_2017_amd import em as gem, synth
    from vanishing_points_2017_amd.runtime import get_runtime
    sizes = RING_SEQUENCES[name]
    rt, rt_ref = get_runtime(0, "ring_wrap_" + name), get_runtime(0, "ring_wrap_ref")
    p = gem._params({})
    scenes = [synth.make_scene(seed, 12) for seed in range(97)]
    ds = {n: gem.upload_batch(rt_ref, scenes[:n]) for n in sorted(set(sizes))}
    rt_ref.synchronize()

    def launch(lane, d, keep):
        with lane.on_stream():
            l = d["l"].clone()
        keep.append(l)
        return gem.em_batch_device(lane, d["offsets"], l, d["lp"], d["cnn"], d["sphere"], None, p)

    def host(o):
        return {k: o[k].cpu().numpy() for k in ("vp", "num_vp", "vp_assoc", "status")}

    keep, ref = [], {}
    for n, d in ds.items():                # alone and synchronised, on another lane: this one's buffers stay untouched
        o = launch(rt_ref, d, keep)
        rt_ref.synchronize()
        ref[n] = host(o)
    assert not ref[97]["status"].all() and ref[97]["num_vp"].max() > 0, "images of 12 lines that the EM refines"
    outs = [launch(rt, ds[n], keep) for n in sizes]
    rt.synchronize()
    for k, (n, o) in enumerate(zip(sizes, outs)):
        got = host(o)
        for key in ("status", "num_vp", "vp_assoc", "vp"):      # whole arrays: the EM writes every row of every image
            assert np.array_equal(got[key], ref[n][key], equal_nan=True), (k, n, key)


def test_workspace_bytes_is_the_launch_plans():
    """vpk_em_workspace_bytes answers from csrc/em_plan.hpp: slots x slot bytes of the host build of the plan
    (tests/hostsim/sim_em_plan.cpp), fed with the device's CU count and memory."""
    import ctypes
    from hostsim import simlib_em_plan as sim
    from vanishing_points_2017_amd import em as gem
    from vanishing_points_2017_amd.runtime import get_runtime
    rt = get_runtime(0, "plan_bytes")          # a lane of its own: no workgroup cap, no shared state touched
    info = rt.handle.device_info()
    f = sim.facts(cu_share=info["num_cu"], total_mem=info["hbm_gib"] << 30)
    p = gem._params({})
    for batch, n_max in ((3, 12), (300, 380)):
        w = sim.workspace(f, batch, n_max)
        assert w.slots == min(batch, info["num_cu"]) and w.ws_bytes == w.slots * w.slot_bytes
        assert rt.lib.vpk_em_workspace_bytes(rt.h, batch, n_max, ctypes.byref(p), 0) == w.ws_bytes
