"""ppf_prep_frame's C-ABI surface without a GPU: the two structs as a C compiler lays them out equal their ctypes
mirrors, the defaults are the C1 golden's parameters, argument errors come before any device work and the call fails
loudly (PPF_ERR_HIP) when there is no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import FrameParams, FrameStats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "fsz.c"
    fields_p = ["leaf", "mean_k", "stddev_mul", "normal_k", "curvature_threshold", "flags", "reserved"]
    fields_s = ["n_boxes", "n_launches", "n_host_syncs", "ms_wall", "reserved"]
    expr = ["sizeof(ppf_frame_params)"] + [f"offsetof(ppf_frame_params, {f})" for f in fields_p] + \
           ["sizeof(ppf_frame_stats)"] + [f"offsetof(ppf_frame_stats, {f})" for f in fields_s]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppf_hip.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "fsz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    got = [C.sizeof(FrameParams)] + [getattr(FrameParams, f).offset for f in fields_p] + \
          [C.sizeof(FrameStats)] + [getattr(FrameStats, f).offset for f in fields_s]
    assert got == want


def test_default_frame_params():
    p = FrameParams()
    p.flags = 7
    lib().ppf_default_frame_params(C.byref(p))
    assert (p.leaf, p.mean_k, p.stddev_mul, p.normal_k) == (0.003, 50, 1.0, 30)
    assert p.curvature_threshold == pytest.approx(0.03) and p.flags == 0 and list(p.reserved) == [0, 0, 0, 0]


def _call(scene, boxes, params, depth=None, n_boxes=None, objects=True):
    depth = np.zeros((20, 30), np.float32) if depth is None else depth
    b = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 4))
    nb = b.shape[0] if n_boxes is None else n_boxes
    intr = (C.c_double * 4)(100.0, 100.0, 15.0, 10.0)
    objs = (C.c_void_p * 300)(*([0x1234] * 300))   # garbage the call must overwrite with NULL
    edges = (C.c_void_p * 300)(*([0x1234] * 300))
    st = FrameStats()
    s = lib().ppf_prep_frame(scene, b.ctypes.data_as(C.POINTER(C.c_int)), nb, depth.ctypes.data, depth.shape[0], depth.shape[1],
                             intr, C.byref(params) if params is not None else None, objs if objects else None, edges, None,
                             C.byref(st))
    return s, objs, edges, st


def test_argument_errors_precede_any_device_work():
    dummy = C.create_string_buffer(64)   # never dereferenced: every check below fails before the scene is used
    p = FrameParams()
    lib().ppf_default_frame_params(C.byref(p))
    assert _call(dummy, [[1, 1, 3, 3]], p, objects=False)[0] == _capi.PPF_ERR_INVALID
    assert _call(dummy, [[1, 1, 3, 3]], p, n_boxes=257)[0] == _capi.PPF_ERR_INVALID
    assert _call(dummy, [[1, 1, 3, 3]], p, n_boxes=-1)[0] == _capi.PPF_ERR_INVALID
    assert _call(None, [[1, 1, 3, 3]], p)[0] == _capi.PPF_ERR_INVALID
    assert _call(dummy, [[1, 1, 3, 3]], None)[0] == _capi.PPF_ERR_INVALID
    for field, bad in (("leaf", 0.0), ("leaf", -1.0), ("mean_k", 0), ("mean_k", 64), ("normal_k", 0), ("normal_k", 65)):
        q = FrameParams()
        lib().ppf_default_frame_params(C.byref(q))
        setattr(q, field, bad)
        s, objs, edges, _ = _call(dummy, [[1, 1, 3, 3], [2, 2, 3, 3]], q)
        assert s == _capi.PPF_ERR_INVALID, (field, bad)
        assert not objs[0] and not objs[1] and not edges[0] and not edges[1]   # no handle, not even a stale pointer
        assert objs[2] == 0x1234                                                # nothing beyond n_boxes is touched


def test_frame_without_a_device_is_loud():
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    dummy = C.create_string_buffer(64)
    p = FrameParams()
    lib().ppf_default_frame_params(C.byref(p))
    for boxes in ([[1, 1, 3, 3]], np.zeros((0, 4), np.int32)):
        s, objs, _, st = _call(dummy, boxes, p)
        assert s == _capi.PPF_ERR_HIP
        assert "no HIP device" in _capi.last_error() and "ppf_prep_frame" in _capi.last_error()
        assert not objs[0] if len(boxes) else objs[0] == 0x1234
        assert st.n_launches == 0 and st.n_host_syncs == 0
