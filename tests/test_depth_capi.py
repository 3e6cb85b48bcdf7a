"""ppf_cloud_from_depth's C-ABI surface without a GPU: ppf_depth_params as a C compiler lays it out equals its ctypes
mirror, the defaults, every argument error comes before any device work (and leaves *out NULL), the call fails loudly
(PPF_ERR_HIP) when there is no device, and examples/depth_frame_demo.cpp compiles as C++11."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import DepthParams, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
INTR = (1000.0, 1001.0, 640.5, 360.25)
FIELDS = ["format", "flags", "depth_scale", "z_min", "z_max", "reserved"]


def test_depth_params_layout_matches_the_header(tmp_path):
    src = tmp_path / "dsz.c"
    expr = ["sizeof(ppf_depth_params)"] + [f"offsetof(ppf_depth_params, {f})" for f in FIELDS] + \
           ["PPF_DEPTH_F32", "PPF_DEPTH_U16", "PPF_DEPTH_FP64", "PPF_ABI_VERSION"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppf_hip.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "dsz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    got = [C.sizeof(DepthParams)] + [getattr(DepthParams, f).offset for f in FIELDS] + \
          [_capi.PPF_DEPTH_F32, _capi.PPF_DEPTH_U16, _capi.PPF_DEPTH_FP64, _capi.PPF_ABI_VERSION]
    assert got == want


def defaults():
    p = DepthParams()
    p.format, p.flags, p.depth_scale, p.z_min, p.z_max = 7, 7, 7.0, 7.0, 7.0
    for i in range(4):
        p.reserved[i] = 7
    lib().ppf_default_depth_params(C.byref(p))
    return p


def test_defaults():
    p = defaults()
    assert (p.format, p.flags, p.depth_scale, p.z_min, p.z_max) == (_capi.PPF_DEPTH_F32, 0, 0.001, 0.0, 0.0)
    assert list(p.reserved) == [0, 0, 0, 0]
    lib().ppf_default_depth_params(None)   # no crash


SENTINEL = 0x5A5A5A5A


def host_call(img, rows, cols, pitch=0, intr=INTR, p=None, out=True):
    it = (C.c_double * 4)(*intr) if intr is not None else None
    prm = defaults() if p is None else p
    o = C.c_void_p(SENTINEL)
    s = lib().ppf_cloud_from_depth(C.c_void_p(img.ctypes.data) if img is not None else None, rows, cols, pitch, it,
                                   C.byref(prm) if prm is not False else None, C.byref(o) if out else None)
    return s, o.value


def device_call(rows, cols, pitch=0, intr=INTR, p=None, ptr=0x10):
    """the device entry with arguments that are rejected before the pointer is looked at (ptr is never read)"""
    it = (C.c_double * 4)(*intr) if intr is not None else None
    prm = defaults() if p is None else p
    o = C.c_void_p(SENTINEL)
    s = lib().ppf_cloud_from_depth_device(C.c_void_p(ptr) if ptr else None, rows, cols, pitch, it, C.byref(prm), None, C.byref(o))
    return s, o.value


def params(**kw):
    p = defaults()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def bad_cases():
    f32 = np.zeros((4, 6), np.float32)
    u16 = np.zeros((4, 6), np.uint16)
    odd = np.zeros(64, np.uint8)[1:]   # an image one byte past its elements' alignment
    return [
        ("NULL depth", dict(img=None, rows=4, cols=6)),
        ("NULL intr", dict(img=f32, rows=4, cols=6, intr=None)),
        ("NULL params", dict(img=f32, rows=4, cols=6, p=False)),
        ("rows 0", dict(img=f32, rows=0, cols=6)),
        ("cols -1", dict(img=f32, rows=4, cols=-1)),
        ("rows * cols > INT32_MAX", dict(img=f32, rows=65536, cols=32768)),
        ("pitch below the row", dict(img=f32, rows=4, cols=6, pitch=20)),
        ("pitch not a multiple", dict(img=f32, rows=4, cols=6, pitch=26)),
        ("u16 pitch odd", dict(img=u16, rows=4, cols=6, pitch=13, p=params(format=_capi.PPF_DEPTH_U16))),
        ("misaligned image", dict(img=odd, rows=2, cols=3, p=params(format=_capi.PPF_DEPTH_U16))),
        ("format 2", dict(img=f32, rows=4, cols=6, p=params(format=2))),
        ("format -1", dict(img=f32, rows=4, cols=6, p=params(format=-1))),
        ("unknown flag", dict(img=f32, rows=4, cols=6, p=params(flags=2))),
        ("u16 scale 0", dict(img=u16, rows=4, cols=6, p=params(format=_capi.PPF_DEPTH_U16, depth_scale=0.0))),
        ("u16 scale < 0", dict(img=u16, rows=4, cols=6, p=params(format=_capi.PPF_DEPTH_U16, depth_scale=-0.001))),
        ("u16 scale nan", dict(img=u16, rows=4, cols=6, p=params(format=_capi.PPF_DEPTH_U16, depth_scale=math.nan))),
        ("fx 0", dict(img=f32, rows=4, cols=6, intr=(0.0, 1.0, 2.0, 2.0))),
        ("fy 0", dict(img=f32, rows=4, cols=6, intr=(1.0, -0.0, 2.0, 2.0))),
        ("fx inf", dict(img=f32, rows=4, cols=6, intr=(math.inf, 1.0, 2.0, 2.0))),
        ("fy nan", dict(img=f32, rows=4, cols=6, intr=(1.0, math.nan, 2.0, 2.0))),
        ("ppx nan", dict(img=f32, rows=4, cols=6, intr=(1.0, 1.0, math.nan, 2.0))),
        ("z_min inf", dict(img=f32, rows=4, cols=6, p=params(z_min=math.inf))),
        ("z_max < 0", dict(img=f32, rows=4, cols=6, p=params(z_max=-1.0))),
    ]


@pytest.mark.parametrize("name,kw", bad_cases(), ids=[c[0] for c in bad_cases()])
def test_argument_errors_precede_any_device_work(name, kw):
    s, out = host_call(**kw)
    assert s == _capi.PPF_ERR_INVALID, (name, _capi.last_error())
    assert out is None, name                               # *out set to NULL
    assert "ppf_cloud_from_depth" in _capi.last_error()


def test_device_entry_argument_errors_precede_any_device_work():
    cases = [dict(rows=4, cols=6, ptr=0), dict(rows=0, cols=6), dict(rows=4, cols=6, pitch=8), dict(rows=4, cols=6, p=params(format=3)),
             dict(rows=4, cols=6, intr=(1.0, 0.0, 1.0, 1.0)), dict(rows=4, cols=6, intr=None),
             dict(rows=4, cols=6, p=params(format=_capi.PPF_DEPTH_U16, depth_scale=0.0)), dict(rows=1 << 16, cols=1 << 15)]
    for kw in cases:
        s, out = device_call(**kw)
        assert s == _capi.PPF_ERR_INVALID and out is None, (kw, _capi.last_error())
        assert "ppf_cloud_from_depth_device" in _capi.last_error()
    it = (C.c_double * 4)(*INTR)
    assert lib().ppf_cloud_from_depth_device(C.c_void_p(0x10), 4, 6, 0, it, C.byref(defaults()), None, None) == _capi.PPF_ERR_INVALID
    assert lib().ppf_cloud_from_depth(None, 4, 6, 0, it, C.byref(defaults()), None) == _capi.PPF_ERR_INVALID


def test_from_depth_without_a_device_is_loud():
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    img = np.ones((4, 6), np.float32)
    s, out = host_call(img, 4, 6)
    assert s == _capi.PPF_ERR_HIP and out is None
    assert "no HIP device" in _capi.last_error() and "ppf_cloud_from_depth" in _capi.last_error()
    s, out = device_call(4, 6)
    assert s == _capi.PPF_ERR_HIP and out is None
    u16 = np.ones((4, 6), np.uint16)
    assert host_call(u16, 4, 6, p=params(format=_capi.PPF_DEPTH_U16, flags=_capi.PPF_DEPTH_FP64))[0] == _capi.PPF_ERR_HIP


def test_python_wrapper_rejects_other_dtypes():
    from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud
    for bad in (np.zeros((4, 6), np.float64), np.zeros((4, 6, 1), np.float32), np.zeros(6, np.uint16)):
        with pytest.raises(_capi.PPFError) as e:
            DeviceCloud.from_depth(bad, INTR)
        assert e.value.status == _capi.PPF_ERR_INVALID


def _build(tmp_path, std="c++11", with_opencv_stand_in=False):
    exe = str(tmp_path / ("depth_frame_demo" + ("_cv" if with_opencv_stand_in else "")))
    inc = ["-I", os.path.join(ROOT, "include")] + (["-I", os.path.join(ROOT, "tests", "mock_opencv")] if with_opencv_stand_in else [])
    subprocess.run(["g++", f"-std={std}", "-Wall", "-Wextra", "-Werror"] + inc +
                   [os.path.join(ROOT, "examples", "depth_frame_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe],
                   check=True)
    return exe


def test_depth_frame_demo_compiles_as_cxx11_with_and_without_the_opencv_stand_in(tmp_path):
    _build(tmp_path)
    _build(tmp_path, with_opencv_stand_in=True)


def test_depth_frame_demo_fails_loudly_without_gpu(tmp_path):
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    exe = _build(tmp_path)
    (tmp_path / "d.f32").write_bytes(np.ones((4, 6), np.float32).tobytes())
    (tmp_path / "m.f32").write_bytes(np.ones((3, 6), np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "d.f32"), "4", "6"] + [repr(v) for v in INTR] + ["none", "0", str(tmp_path / "m.f32"), "3"],
                       capture_output=True, text=True)
    assert r.returncode == 10 + _capi.PPF_ERR_HIP, (r.returncode, r.stderr)
    assert "ppf_cloud_from_depth" in r.stderr
