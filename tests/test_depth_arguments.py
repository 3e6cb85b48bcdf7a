"""The one depth-argument path of cloud_processor.py without a GPU: what _DepthInput hands to an entry for numpy images
and CPU tensors (pointer, rows, cols, pitch in bytes, format), which views are read in place and which are copied, what
_DepthInput.output makes or refuses, _depth_params, and the PPFError texts of the five functions that go through them
(DeviceCloud.from_depth, DepthMap.register, filter_depth, DepthHistory.push, segment_depth)."""
import numpy as np
import pytest
import torch

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.cloud_processor import (DepthHistory, DepthMap, DeviceCloud, _depth_params, _DepthInput, filter_depth,
                                                          segment_depth)

TWO_D = "depth must be a 2-D float32 or uint16 {kind}"
INTR = (500.0, 500.0, 3.0, 2.0)


def handed(inp):
    return inp.ptr.value, inp.rows, inp.cols, inp.pitch, inp.format


@pytest.mark.parametrize("dtype,fmt", [(np.float32, _capi.PPF_DEPTH_F32), (np.uint16, _capi.PPF_DEPTH_U16)])
def test_packed_and_row_strided_images_are_read_in_place(dtype, fmt):
    wide = np.arange(4 * 9, dtype=dtype).reshape(4, 9)
    inp = _DepthInput(wide, TWO_D)
    assert handed(inp) == (wide.ctypes.data, 4, 9, 9 * wide.itemsize, fmt) and inp.keep is wide
    assert not inp.is_device and inp.shape == (4, 9)
    view = wide[:, :5]                                                   # keeps the wide array's pitch: no copy
    inp = _DepthInput(view, TWO_D)
    assert handed(inp) == (wide.ctypes.data, 4, 5, 9 * wide.itemsize, fmt) and inp.keep is view
    inner = wide[1:, 2:7]
    assert handed(_DepthInput(inner, TWO_D)) == (wide.ctypes.data + (9 + 2) * wide.itemsize, 3, 5, 9 * wide.itemsize, fmt)
    with inp.device():                                                   # nothing to select for a host image
        pass


@pytest.mark.parametrize("dtype,fmt", [(np.float32, _capi.PPF_DEPTH_F32), (np.uint16, _capi.PPF_DEPTH_U16)])
def test_views_whose_strides_are_no_row_strides_are_copied(dtype, fmt):
    wide = np.arange(4 * 10, dtype=dtype).reshape(4, 10)
    for view in (wide[:, ::2], wide.T, wide[::-1], np.broadcast_to(wide[0], (4, 10))):
        inp = _DepthInput(view, TWO_D)
        rows, cols = view.shape
        assert handed(inp) == (inp.keep.ctypes.data, rows, cols, cols * wide.itemsize, fmt)
        assert inp.keep is not view and inp.keep.flags.c_contiguous and np.array_equal(inp.keep, view)
        assert not np.shares_memory(inp.keep, wide)


def test_a_cpu_tensor_goes_the_numpy_way():
    t = torch.arange(4 * 9, dtype=torch.float32).reshape(4, 9)
    inp = _DepthInput(t[:, :5], TWO_D)
    assert handed(inp) == (t.data_ptr(), 4, 5, 36, _capi.PPF_DEPTH_F32) and not inp.is_device and isinstance(inp.keep, np.ndarray)
    out, ptr = inp.output(None, np.float32)
    assert isinstance(out, np.ndarray) and ptr.value == out.ctypes.data


@pytest.mark.parametrize("bad", [np.ones((4, 6), np.float64), np.ones((4, 6), np.int16), np.ones((4, 6), ">f4"), np.ones((2, 4, 6), np.float32),
                                 np.ones(6, np.float32), np.float32(1.0), None, torch.ones(4, 6, dtype=torch.float64)],
                         ids=["float64", "int16", "big-endian", "3-D", "1-D", "0-D", "None", "cpu float64 tensor"])
def test_other_dtypes_and_ranks_are_refused_with_the_callers_text(bad):
    with pytest.raises(_capi.PPFError) as e:
        _DepthInput(bad, TWO_D)
    assert e.value.status == _capi.PPF_ERR_INVALID and "depth must be a 2-D float32 or uint16 array" in str(e.value)


def test_a_required_shape_and_dtype():
    img = np.ones((4, 6), np.float32)
    assert _DepthInput(img, "x {kind}", shape=(4, 6), dtype=np.dtype(np.float32)).shape == (4, 6)
    for kw in (dict(shape=(6, 4)), dict(shape=(4, 7)), dict(dtype=np.dtype(np.uint16)), dict(shape=(4, 6), dtype=np.dtype(np.uint16))):
        with pytest.raises(_capi.PPFError) as e:
            _DepthInput(img, "depth must be a uint16 {kind} of shape (6, 4)", **kw)
        assert e.value.status == _capi.PPF_ERR_INVALID and "depth must be a uint16 array of shape (6, 4)" in str(e.value)


def test_output_makes_or_validates():
    inp = _DepthInput(np.ones((4, 9), np.float32)[:, :5], TWO_D)
    out, ptr = inp.output(None, np.float32)
    assert out.shape == (4, 5) and out.dtype == np.float32 and out.flags.c_contiguous and ptr.value == out.ctypes.data
    lab, _ = inp.output(None, np.int32)
    assert lab.dtype == np.int32 and lab.shape == (4, 5)
    big, _ = inp.output(None, np.float32, (7, 8))
    assert big.shape == (7, 8)
    mine = np.zeros((4, 5), np.float32)
    got, ptr = inp.output(mine, np.float32)
    assert got is mine and ptr.value == mine.ctypes.data
    ro = np.zeros((4, 5), np.float32)
    ro.setflags(write=False)
    bad = {"dtype": np.zeros((4, 5), np.float64), "shape": np.zeros((5, 4), np.float32), "non-contiguous": np.zeros((4, 10), np.float32)[:, ::2],
           "read-only": ro, "a list": [[0.0] * 5] * 4, "a tensor": torch.zeros(4, 5)}
    for name, o in bad.items():
        with pytest.raises(_capi.PPFError) as e:
            inp.output(o, np.float32)
        assert e.value.status == _capi.PPF_ERR_INVALID and "out must be a contiguous float32 array of shape (4, 5)" in str(e.value), name
    with pytest.raises(_capi.PPFError) as e:
        inp.output(mine, np.int32)
    assert "out must be a contiguous int32 array of shape (4, 5)" in str(e.value)


def test_depth_params():
    dp = _depth_params(0.002, 0.25, 3.5)
    assert (dp.format, dp.flags, dp.depth_scale, dp.z_min, dp.z_max) == (_capi.PPF_DEPTH_F32, 0, 0.002, 0.25, 3.5) and list(dp.reserved) == [0] * 4
    assert _depth_params(1, 0, 0, _capi.PPF_DEPTH_FP64).flags == _capi.PPF_DEPTH_FP64


def test_the_five_functions_keep_their_texts():
    f64, cube, img = np.ones((4, 6), np.float64), np.ones((2, 4, 6), np.float32), np.ones((4, 6), np.float32)
    two_d = "depth must be a 2-D float32 or uint16 array"
    hist, dmap = DepthHistory.__new__(DepthHistory), DepthMap.__new__(DepthMap)           # no device: the handles are never reached
    hist._ptr, hist.shape, hist.dtype = None, (4, 6), np.dtype(np.uint16)
    dmap._ptr, dmap.depth_shape, dmap.color_shape = None, (4, 6), (8, 9)
    ro = np.zeros((4, 6), np.float32)
    ro.setflags(write=False)
    cases = [
        (lambda: DeviceCloud.from_depth(f64, INTR), two_d),
        (lambda: DeviceCloud.from_depth(cube, INTR, normals={}), two_d),
        (lambda: filter_depth(f64), two_d),
        (lambda: filter_depth(cube), two_d),
        (lambda: segment_depth(f64), two_d),
        (lambda: segment_depth(cube), two_d),
        (lambda: dmap.register(f64), "depth must be a float32 or uint16 array of shape (4, 6)"),
        (lambda: dmap.register(np.ones((6, 4), np.float32)), "depth must be a float32 or uint16 array of shape (4, 6)"),
        (lambda: hist.push(img), "depth must be a uint16 array of shape (4, 6)"),
        (lambda: hist.push(np.ones((4, 7), np.uint16)), "depth must be a uint16 array of shape (4, 6)"),
        (lambda: filter_depth(img, out=np.zeros((4, 6), np.float64)), "out must be a contiguous float32 array of shape (4, 6)"),
        (lambda: filter_depth(img, out=np.zeros((4, 7), np.float32)), "out must be a contiguous float32 array of shape (4, 6)"),
        (lambda: filter_depth(img, out=np.zeros((4, 12), np.float32)[:, ::2]), "out must be a contiguous float32 array of shape (4, 6)"),
        (lambda: filter_depth(img, out=ro), "out must be a contiguous float32 array of shape (4, 6)"),
        (lambda: segment_depth(img, out=np.zeros((4, 6), np.float32)), "out must be a contiguous int32 array of shape (4, 6)"),
        (lambda: hist.push(np.ones((4, 6), np.uint16), out=np.zeros((6, 4), np.float32)), "out must be a contiguous float32 array of shape (4, 6)"),
    ]
    for k, (call, text) in enumerate(cases):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID and text in str(e.value), (k, str(e.value))
