"""The float-image surface of the CNN without a GPU: the C-ABI declarations and bindings, the dtype dispatch (cnn.image_kind)
and the shape check that runs before any device work."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_header_declares_the_float_entry_points():
    from vanishing_points_2017_amd import _lib
    text = open(os.path.join(ROOT, "include", "vpk.h")).read()
    for sym, args in (("vpk_cnn_forward_f32", "vpk_handle* h, const float* image, int batch, float* out"),
                      ("vpk_cnn_forward_tap_f32", "vpk_handle* h, const float* image, int batch, float* out, int tap, float* tap_out")):
        assert "int %s(%s);" % (sym, args) in text, sym
        assert sym in _lib.EXPORTS
    assert "replaces: caffe_forward (evaluation.py:34-38) for float images" in text


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
def test_float_dtypes_take_the_float_path(dtype):
    from vanishing_points_2017_amd import cnn
    assert cnn.image_kind(np.zeros((2, 500, 500), dtype)) == "f32"
    assert cnn.image_kind(np.zeros((500, 500), dtype)) == "f32"
    assert cnn.image_kind(torch.zeros((3, 500, 500), dtype=getattr(torch, np.dtype(dtype).name))) == "f32"


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.int32, np.int64, np.uint16, np.bool_])
def test_every_other_dtype_keeps_the_uint8_path(dtype):
    from vanishing_points_2017_amd import cnn
    assert cnn.image_kind(np.zeros((2, 500, 500), dtype)) == "u8"
    assert cnn.image_kind(torch.zeros((2, 500, 500), dtype=torch.uint8)) == "u8"
    assert cnn.image_kind([[0, 1], [2, 3]]) == "u8"              # (anything np.asarray takes; the uint8 cast decides as before)
    assert cnn.image_kind(np.zeros((7,), dtype)) == "u8"         # (no shape rule for the uint8 path: unchanged)


@pytest.mark.parametrize("shape", [(500,), (2, 500, 499), (500, 500, 1), (1, 1, 500, 500), (250000,), (499, 500)])
def test_float_images_of_the_wrong_shape_are_refused(shape):
    from vanishing_points_2017_amd import cnn
    with pytest.raises(ValueError):
        cnn.image_kind(np.zeros(shape, np.float32))
    with pytest.raises(ValueError):
        cnn.image_kind(torch.zeros(shape, dtype=torch.float64))


class _NoDevice(object):
    """A runtime whose every use is an error: what a Net touches before its shape check."""
    def __getattr__(self, name):
        raise AssertionError("device work before the shape check: rt.%s" % name)


def test_the_shape_check_comes_before_any_device_work():
    from vanishing_points_2017_amd import cnn
    net = object.__new__(cnn.Net)
    net.rt = _NoDevice()
    net._last_batch = None
    bad = np.zeros((2, 500, 499), np.float32)
    with pytest.raises(ValueError):
        net.forward(bad)
    with pytest.raises(ValueError):
        net.forward_device(torch.zeros((2, 500, 499)))
    with pytest.raises(ValueError):
        net.forward_device(torch.zeros((500, 500)))             # forward_device takes batches only
    with pytest.raises(ValueError):
        cnn.caffe_forward(net, np.zeros((500, 501), np.float64))
    lazy = cnn.LazyNet({})
    lazy._net = net
    with pytest.raises(ValueError):
        lazy.forward_batch(np.zeros((3, 400, 500), np.float16))
