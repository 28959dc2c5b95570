"""The range policy's host surface (no GPU): the policy names, the error code, the C-ABI declarations and their Python bindings."""
import os
import re

import pytest

from conftest import ROOT


def test_policy_names_map_to_the_abi_values():
    from vanishing_points_2017_amd import cnn
    assert cnn.range_policy_code("raise") == 0
    assert cnn.range_policy_code("recompute_exact") == 1
    for bad in ("RAISE", "exact", None, 1):
        with pytest.raises(ValueError):
            cnn.range_policy_code(bad)
    with pytest.raises(ValueError):                      # checked before anything touches a GPU
        cnn.LazyNet({}, range_policy="clamp")


def test_range_error_code_is_defined_once():
    from vanishing_points_2017_amd import _lib
    assert _lib.VPK_ERR_RANGE == -6
    pkg = os.path.join(ROOT, "vanishing_points_2017_amd")
    for name in ("cnn.py", "pipeline.py"):
        src = open(os.path.join(pkg, name)).read()
        assert not re.search(r"==\s*-6\b|\(0,\s*-6\)|error -6", src), name


def test_header_declares_the_policy_entry_points():
    from vanishing_points_2017_amd import _lib
    text = open(os.path.join(ROOT, "include", "vpk.h")).read()
    for sym, args in (("vpk_cnn_set_range_policy", "vpk_handle* h, int policy"),
                      ("vpk_cnn_image_range_flags", "vpk_handle* h, int batch, uint32_t* flags_out"),
                      ("vpk_cnn_recomputed", "vpk_handle* h, int64_t* n_out")):
        assert "int %s(%s);" % (sym, args) in text, sym
        assert sym in _lib.EXPORTS
    assert re.search(r"#define VPK_VERSION 110\b", text)


def test_entry_points_take_the_keyword_with_the_default():
    import inspect
    from vanishing_points_2017_amd import evaluation, pipeline
    for fn, positional in ((evaluation.init_caffe, ["model_def", "model_weights", "gpu_id", "mean_file"]),
                           (evaluation.run_cnn, ["dataset", "model_def", "model_weights", "mean_file", "gpu", "net"])):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[:len(positional)] == positional
        assert sig.parameters["range_policy"].default == "raise"
    assert inspect.signature(pipeline.Step.__init__).parameters["range_policy"].default is None
