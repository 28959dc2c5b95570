"""EM-only timing of the 102 YUD-shape scenes (the bench's batch) under each distance measure of the EM (dev tool):
one vpk_em_batch launch per repetition, timed with stream events, best of the repetitions after a warm-up."""
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402
from vanishing_points_2017_amd import em as gem, synth  # noqa: E402
from vanishing_points_2017_amd.runtime import get_runtime  # noqa: E402

rt = get_runtime(0)
scenes = list(synth.config_scenes(2))
d = gem.upload_batch(rt, scenes)
l0 = d["l"].clone()
p = gem._params({})
for measure in ("angle", "dotprod", "angle", "dotprod"):
    ts = []
    for rep in range(5):
        d["l"].copy_(l0)
        rt.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with rt.on_stream():
            e0.record()
            out = gem.em_batch_device(rt, d["offsets"], d["l"], d["lp"], d["cnn"], d["sphere"], None, p, distance_measure=measure)
            e1.record()
        rt.synchronize()
        ts.append(e0.elapsed_time(e1))
    it, m = out["iterations"].cpu().numpy(), out["num_vp"].cpu().numpy()
    print("%-8s %d images: best %.2f ms (all: %s), iterations mean %.1f max %d, VPs mean %.1f, status %s" % (
        measure, len(scenes), min(ts[1:]), " ".join("%.2f" % t for t in ts), it.mean(), it.max(), m.mean(),
        np.bincount(out["status"].cpu().numpy())), flush=True)
