"""Net.forward_device on a float device tensor that the caller's stream is still writing.

The handle's stream is non-blocking: nothing orders it behind torch's current stream by itself.  A caller that converts
images to float on its own stream and hands the result straight to forward_device (tests/test_gpu_cnn_float_input.py does,
with 8 GB at B = 4097) therefore needs forward_device to wait for that stream, or the forward reads the tensor before it is
written.  Here the caller's stream is held back by a spin kernel of a few milliseconds in front of the write, so that the
order decides the result every time: without the wait the forward sees the zeros the tensor held before."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_forward_device_waits_for_the_callers_stream():
    import torch
    from vanishing_points_2017_amd import cnn, sphere_mapping, synth
    net = cnn.Net(cnn.synthetic_weights(0), cnn.synthetic_mean(0))
    rt = net.rt
    r = sphere_mapping.raster_batch([s["l"] for s in synth.config_scenes(2, count=2, start=10)])
    d8 = torch.from_numpy(r).to(rt.tdev)
    want = net.forward_device(d8)
    rt.synchronize()
    want = want.cpu().numpy()
    x = torch.zeros(d8.shape, dtype=torch.float32, device=rt.tdev)
    blank = net.forward_device(x)
    rt.synchronize()
    assert not np.array_equal(blank.cpu().numpy(), want)          # (the order below is visible in the result)
    # streams share a few hardware queues, and two streams on one queue run in order by accident: several caller streams,
    # so that at least one does not share the handle's
    for caller in [torch.cuda.Stream(device=rt.tdev) for _ in range(6)]:
        with torch.cuda.stream(caller):
            x.zero_()
            caller.synchronize()
            torch.cuda._sleep(20000000)       # the caller's stream: busy for some milliseconds ...
            x.copy_(d8)                       # ... then the images arrive, on that stream
            got = net.forward_device(x)
            rt.synchronize()
            assert np.array_equal(got.cpu().numpy(), want)
        torch.cuda.synchronize()
