"""CNN forward time at the YUD shape (102 images) under each range policy (include/vpk.h: vpk_cnn_set_range_policy):
"raise", "recompute_exact" with no image flagged, and "recompute_exact" with ONE image (the all-255 raster among 101 sparse
ones) flagged by raising one layer's activation scale.  HIP events on the handle's stream around each forward; median of
--iters forwards after --warmup.  Prints one JSON line."""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from vanishing_points_2017_amd import cnn  # noqa: E402
from vanishing_points_2017_amd.runtime import get_runtime  # noqa: E402

args = sys.argv[1:]
iters = int(args[args.index("--iters") + 1]) if "--iters" in args else 50
warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 10
rt = get_runtime(0)
torch = rt.torch
net = cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0), runtime=rt)
rng = np.random.RandomState(5)
host = ((rng.rand(102, 500, 500) < 0.15) * rng.randint(0, 60, (102, 500, 500))).astype(np.uint8)   # sparse, like a few lines
host[51] = 255
x = torch.from_numpy(host).to(rt.tdev)
out = torch.empty((102, 20, 20), dtype=torch.float32, device=rt.tdev)


def timed():
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * iters)]
    with rt.on_stream():
        for _ in range(warmup):
            rt.check(rt.lib.vpk_cnn_forward(rt.h, rt.ptr(x), 102, rt.ptr(out)))
        for i in range(iters):
            ev[2 * i].record(rt.stream)
            rt.check(rt.lib.vpk_cnn_forward(rt.h, rt.ptr(x), 102, rt.ptr(out)))
            ev[2 * i + 1].record(rt.stream)
    rt.synchronize()
    return float(np.median([ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(iters)]))


res = {}
net.set_range_policy("raise")
res["raise_ms"] = timed()
assert net.range_flags() == 0
net.set_range_policy("recompute_exact")
net.recomputed()
res["recompute_none_flagged_ms"] = timed()
assert net.recomputed() == 0
# one flagged image: conv2's input scale raised until the all-255 raster (and only it) leaves fp16's range
good = net.activation_scales()
net.set_range_policy("raise")
_, t = net.forward(host, tap=1)
m = np.abs(t.reshape(102, -1)).max(axis=1) * float(good[0])
e = int(np.ceil(np.log2(2 * 65504.0 / m[51])))
assert (np.delete(m, 51) * 2.0 ** e < 65504.0).all(), "no power of two separates the all-255 raster"
bad = good.copy()
bad[0] = good[0] * np.float32(2.0 ** e)
net.set_activation_scales(bad)
net.set_range_policy("recompute_exact")
net.recomputed()
res["recompute_one_flagged_ms"] = timed()
assert net.recomputed() == warmup + iters
assert (net.image_range_flags(102) != 0).sum() == 1
net.set_activation_scales(good)
net.set_range_policy("raise")
res["added_none_flagged_ms"] = res["recompute_none_flagged_ms"] - res["raise_ms"]
res["added_one_flagged_ms"] = res["recompute_one_flagged_ms"] - res["raise_ms"]
print(json.dumps({k: round(v, 4) for k, v in res.items()}))
