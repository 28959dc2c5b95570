"""vanishing_points_2017_amd/ragged.py on its own: the host part of the batch call surface -- offsets and shape checks --
which needs neither torch, the library nor a GPU."""
import ctypes

import numpy as np
import pytest

from vanishing_points_2017_amd import ragged


def test_offsets_from_sizes():
    off = ragged.offsets_of([5, 0, 3])
    assert off.dtype == np.int64 and off.tolist() == [0, 5, 5, 8]
    assert ragged.offsets_of([]).tolist() == [0] and ragged.offsets_of([]).dtype == np.int64      # an empty batch
    assert ragged.offsets_of([0, 0]).tolist() == [0, 0, 0]                                        # images without lines
    assert ragged.offsets_of(np.array([2, 3]) ** 2).tolist() == [0, 4, 13]
    assert ragged.offsets_of([2 ** 31, 2 ** 31]).tolist() == [0, 2 ** 31, 2 ** 32]
    p = ragged.off_ptr(off)
    assert isinstance(p, ctypes.c_void_p) and p.value == off.ctypes.data


def test_callers_offsets():
    off = ragged.check_offsets([0, 5, 5, 8], 8, "lps offsets")
    assert off.dtype == np.int64 and off.flags.c_contiguous and off.tolist() == [0, 5, 5, 8]
    assert ragged.check_offsets(np.array([0], np.int32), 0, "x").tolist() == [0]
    assert ragged.check_offsets([0, 2, 7], None, "vp_offsets").tolist() == [0, 2, 7]              # no total to end at
    for bad in ([1, 5, 8], [0, 5, 4, 8], [0, 5, 7], [0, 5, 9], [], [[0, 8]], 8):                  # start, step down, total, length
        with pytest.raises(ValueError, match="lps offsets must rise from 0 to 8"):
            ragged.check_offsets(bad, 8, "lps offsets")
    with pytest.raises(ValueError, match=r"^offsets must rise from 0 to the number of lines \(8\)$"):
        ragged.check_offsets([0, 5, 7], 8, "offsets", "the number of lines (8)")
    for bad in ([1, 5], [0, 5, 4], []):
        with pytest.raises(ValueError, match="vp_offsets must rise from 0$"):
            ragged.check_offsets(bad, None, "vp_offsets")


def test_offsets_of_a_list_or_of_a_concatenated_batch():
    arrs = [np.zeros((5, 3)), np.zeros((0, 3)), np.zeros((3, 3))]
    assert ragged.batch_offsets(arrs, None, "ls").tolist() == [0, 5, 5, 8]
    assert ragged.batch_offsets(arrs, [0, 1], "ls").tolist() == [0, 5, 5, 8], "a list's sizes are its own"
    assert ragged.batch_offsets([[1.0, 2.0], []], None, "ss").tolist() == [0, 2, 2]
    assert ragged.batch_offsets([], None, "ls").tolist() == [0]
    cat = np.concatenate(arrs)
    assert ragged.batch_offsets(cat, [0, 5, 5, 8], "ls").tolist() == [0, 5, 5, 8]
    with pytest.raises(ValueError, match="ls is one concatenated array: its offsets are needed"):
        ragged.batch_offsets(cat, None, "ls")
    with pytest.raises(ValueError, match="ls offsets must rise from 0 to 8"):
        ragged.batch_offsets(cat, [0, 5, 7], "ls")
    # the strict form: every image its exact row shape
    assert ragged.strict_offsets(arrs, (3,), "ls").tolist() == [0, 5, 5, 8]
    assert ragged.strict_offsets([np.zeros(2), [1.0]], (), "ss").tolist() == [0, 2, 3]
    for bad in (np.zeros((5, 4)), np.zeros(15), np.zeros((5, 3, 1))):
        with pytest.raises(ValueError, match=r"ls: every image needs shape \(rows, 3\)"):
            ragged.strict_offsets([arrs[0], bad], (3,), "ls")
    with pytest.raises(ValueError, match=r"ss: every image needs shape \(rows,\)"):
        ragged.strict_offsets([np.zeros((2, 1))], (), "ss")


def test_vp_offsets_of_matrices():
    mats = [np.zeros((2, 5)), np.zeros((1, 0)), np.zeros((0, 3))]
    assert ragged.vp_sizes_of_mats(mats, None, "ws").tolist() == [0, 2, 3, 3]
    with pytest.raises(ValueError, match="two-dimensional"):
        ragged.vp_sizes_of_mats([np.zeros(10)], None, "ws")
    flat = np.zeros(10)
    assert ragged.vp_sizes_of_mats(flat, [0, 2, 3, 3], "ws").tolist() == [0, 2, 3, 3]
    with pytest.raises(ValueError, match="vp_offsets is needed"):
        ragged.vp_sizes_of_mats(flat, None, "ws")
    with pytest.raises(ValueError, match="vp_offsets must rise from 0"):
        ragged.vp_sizes_of_mats(flat, [0, 2, 1], "ws")


def test_image_counts_and_limits():
    lo, vo = ragged.offsets_of([5, 0, 3]), ragged.offsets_of([2, 1, 0])
    ragged.check_counts(lo, vo, "ls", "ws")
    with pytest.raises(ValueError, match="ls and ws describe 3 and 2 images"):
        ragged.check_counts(lo, vo[:-1], "ls", "ws")
    ragged.check_counts(ragged.offsets_of([ragged.MAX_LINES]), ragged.offsets_of([ragged.MAX_VP]), "ls", "ws")
    with pytest.raises(ValueError, match="65 VPs: at most 64"):
        ragged.check_counts(lo, ragged.offsets_of([2, 65, 0]), "ls", "ws")
    with pytest.raises(ValueError, match="32769 lines in one image: at most 32768"):
        ragged.check_counts(ragged.offsets_of([5, 0, 32769]), vo, "ls", "ws")
    ragged.check_images(ragged.offsets_of([5, 0, 32769]), vo, "lps", "vs")           # (the VP set functions bound the VPs alone)
    ragged.check_counts(ragged.offsets_of([]), ragged.offsets_of([]), "ls", "ws")    # an empty batch


def test_row_checks():
    lo = ragged.offsets_of([5, 0, 3])
    arrs = [np.zeros((5, 3)), np.zeros((0, 3)), np.zeros((3, 3))]
    ragged.check_rows(arrs, lo, 3, "ls")
    ragged.check_rows(np.zeros((8, 3)), lo, 3, "ls")
    ragged.check_rows(np.zeros(24), lo, 3, "ls")                                     # (element counts: any shape that holds them)
    with pytest.raises(ValueError, match="ls holds 2 images, expected 3"):
        ragged.check_rows(arrs[:2], lo, 3, "ls")
    with pytest.raises(ValueError, match=r"ls\[2\] holds 12 elements, expected 9"):
        ragged.check_rows(arrs[:2] + [np.zeros((4, 3))], lo, 3, "ls")
    with pytest.raises(ValueError, match="ls holds 21 elements, expected 24"):
        ragged.check_rows(np.zeros((7, 3)), lo, 3, "ls")
    # the sum alone, however a list divides it
    ragged.check_total([np.zeros(4), np.zeros(4)], 8, "ss")
    ragged.check_total(np.zeros((8, 3)), 8, "lines", 3, "rows")
    assert ragged.total([np.zeros((2, 3)), [1.0]]) == 7 and ragged.total(np.zeros((2, 3))) == 6 and ragged.total([]) == 0
    with pytest.raises(ValueError, match="ss holds 7 elements, expected 8"):
        ragged.check_total([np.zeros(4), np.zeros(3)], 8, "ss")
    with pytest.raises(ValueError, match="lines holds 7 rows, expected 8"):
        ragged.check_total(np.zeros((7, 3)), 8, "lines", 3, "rows")


def test_matrix_checks():
    lo, vo = ragged.offsets_of([5, 0, 3]), ragged.offsets_of([2, 1, 0])
    assert ragged.mats_total(lo, vo) == 10
    mats = [np.zeros((2, 5)), np.zeros((1, 0)), np.zeros((0, 3))]
    ragged.check_mats(mats, lo, vo, "ws")
    ragged.check_mats([m.T for m in mats], lo, vo, "lvsqs", transposed=True)
    ragged.check_mats(np.zeros(10), lo, vo, "ws")
    # an image without lines or without VPs: an empty matrix of either orientation, or of no orientation at all
    ragged.check_mats([mats[0], np.zeros((0, 1)), np.zeros((3, 0))], lo, vo, "ws")
    ragged.check_mats([mats[0], np.zeros(0), np.zeros((0, 0))], lo, vo, "ws")
    ragged.check_mats([mats[0].T, np.zeros((1, 0)), np.zeros(0)], lo, vo, "lvsqs", transposed=True)
    with pytest.raises(ValueError, match=r"ws\[0\] has shape \(5, 2\), expected \(2, 5\)"):
        ragged.check_mats([mats[0].T] + mats[1:], lo, vo, "ws")
    with pytest.raises(ValueError, match=r"lvsqs\[0\] has shape \(2, 5\), expected \(5, 2\)"):
        ragged.check_mats(mats, lo, vo, "lvsqs", transposed=True)
    with pytest.raises(ValueError, match=r"ws\[1\] has shape \(1, 1\), expected \(1, 0\)"):
        ragged.check_mats([mats[0], np.zeros((1, 1)), mats[2]], lo, vo, "ws")
    with pytest.raises(ValueError, match="ws holds 2 images, expected 3"):
        ragged.check_mats(mats[:2], lo, vo, "ws")
    with pytest.raises(ValueError, match="ws holds 9 elements, the images' M x N sum to 10"):
        ragged.check_mats(np.zeros(9), lo, vo, "ws")
    # one N x N matrix per image
    lsims = [np.zeros((5, 5)), np.zeros((0, 0)), np.zeros((3, 3))]
    ragged.check_lsims(lsims, lo)
    ragged.check_lsims(np.zeros(34), lo)
    for bad in (lsims[:2], [np.zeros((5, 4))] + lsims[1:], np.zeros(33)):
        with pytest.raises(ValueError, match="one N x N matrix per image"):
            ragged.check_lsims(bad, lo)


def test_the_pair_form_is_told_from_a_list():
    class Dev(object):                                              # what the host part reads of a device tensor
        def data_ptr(self):
            return 0
    assert ragged.is_device_pair((Dev(), [0, 3]))
    assert not ragged.is_device_pair([Dev(), [0, 3]]) and not ragged.is_device_pair((np.zeros((3, 4)), [0, 3]))
    assert ragged.is_list([]) and ragged.is_list(()) and not ragged.is_list(np.zeros(3))
