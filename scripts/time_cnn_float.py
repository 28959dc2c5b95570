"""CNN forward time of float images (vpk_cnn_forward_f32) against uint8 rasters (vpk_cnn_forward) at the YUD shape (102
images): the same rasters, once as uint8 and once as float32, under the default arithmetic.  HIP events on the handle's stream
around each forward, the two paths alternating; median of --iters forwards of each after --warmup.  Then conv1's layer time of
each path (vpk_cnn_set_profiling: mean over --iters profiled passes).  Prints one JSON line."""
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from vanishing_points_2017_amd import cnn, sphere_mapping, synth  # noqa: E402
from vanishing_points_2017_amd.runtime import get_runtime  # noqa: E402

args = sys.argv[1:]
iters = int(args[args.index("--iters") + 1]) if "--iters" in args else 50
warmup = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 10
B = 102
rt = get_runtime(0)
torch = rt.torch
net = cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0), runtime=rt)
host = sphere_mapping.raster_batch([s["l"] for s in synth.config_scenes(2, count=B, start=0)])
x8 = torch.from_numpy(host).to(rt.tdev)
x32 = x8.to(torch.float32)
out = torch.empty((B, 20, 20), dtype=torch.float32, device=rt.tdev)
paths = {"uint8": (rt.lib.vpk_cnn_forward, x8), "float32": (rt.lib.vpk_cnn_forward_f32, x32)}

with rt.on_stream():
    for _ in range(warmup):
        for fwd, x in paths.values():
            rt.check(fwd(rt.h, rt.ptr(x), B, rt.ptr(out)))
    ev = {k: [torch.cuda.Event(enable_timing=True) for _ in range(2 * iters)] for k in paths}
    for i in range(iters):
        for k, (fwd, x) in paths.items():
            ev[k][2 * i].record(rt.stream)
            rt.check(fwd(rt.h, rt.ptr(x), B, rt.ptr(out)))
            ev[k][2 * i + 1].record(rt.stream)
rt.synchronize()
net.check_range()
res = {k + "_ms": float(np.median([e[2 * i].elapsed_time(e[2 * i + 1]) for i in range(iters)])) for k, e in ev.items()}
res["float_over_uint8"] = res["float32_ms"] / res["uint8_ms"]
for k, (fwd, x) in paths.items():
    net.set_profiling(True)            # (restarts the mean)
    with rt.on_stream():
        for _ in range(iters):
            rt.check(fwd(rt.h, rt.ptr(x), B, rt.ptr(out)))
    rt.synchronize()
    ms, n = net.mean_layer_ms()
    net.set_profiling(False)
    res[k + "_conv1_ms"] = ms["conv1"]
    res[k + "_profiled_total_ms"] = sum(ms.values())
print(json.dumps({k: round(v, 4) for k, v in res.items()}))
