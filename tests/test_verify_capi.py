"""ppf_verify_frame's C-ABI surface without a GPU: the three structs as a C compiler lays them out equal their ctypes
mirrors, the defaults, every argument error comes before any device work (with zeroed score rows and best == -1), and a
valid call fails loudly (PPF_ERR_HIP) when there is no device."""
import ctypes as C
import os
import subprocess

import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import FrameDetection, Pose, PoseScore, VerifyParams, VerifyStats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTR = (1000.0, 1001.0, 640.5, 360.25)
NAN, INF = float("nan"), float("inf")


def test_verify_struct_layouts_match_the_header(tmp_path):
    structs = [("ppf_verify_params", VerifyParams), ("ppf_pose_score", PoseScore), ("ppf_verify_stats", VerifyStats)]
    expr, got = [], []
    for cname, cls in structs:
        expr.append(f"sizeof({cname})")
        got.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            expr.append(f"offsetof({cname}, {f})")
            got.append(getattr(cls, f).offset)
    expr += ["PPF_VERIFY_ALL_ROWS", "PPF_VERIFY_NORMALS", "PPF_ABI_VERSION"]
    got += [_capi.PPF_VERIFY_ALL_ROWS, _capi.PPF_VERIFY_NORMALS, 4]
    src = tmp_path / "vsz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppf_hip.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "vsz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want


def defaults():
    p = VerifyParams()
    p.inlier_dist, p.normal_cos, p.depth_tol, p.model_step, p.flags = 7.0, 7.0, 7.0, 7, 7
    for i in range(4):
        p.reserved[i] = 7
    lib().ppf_default_verify_params(C.byref(p))
    return p


def test_defaults():
    p = defaults()
    assert (p.inlier_dist, p.normal_cos, p.depth_tol, p.model_step, p.flags) == (C.c_float(0.005).value, 0.5, C.c_float(0.01).value, 1, 0)
    assert list(p.reserved) == [0, 0, 0, 0]
    lib().ppf_default_verify_params(None)   # no crash


def _dets(n, model_cloud=True, scene=True):
    dummy = C.create_string_buffer(64)   # never dereferenced: every check below fails before a handle is used
    arr = (FrameDetection * 300)()
    for i in range(n):
        arr[i].model_cloud = C.addressof(dummy) if model_cloud else None
        arr[i].scene = C.addressof(dummy) if scene else None
    arr._keep = dummy
    return arr


def _call(dets, n_dets, n_poses=None, top=4, depth=None, rows=0, cols=0, intr=INTR, p=None, poses=True, counts=True, scores=True,
          best=True, params=True):
    np_ = (C.c_int * 300)(*([2] * 300 if n_poses is None else n_poses))
    ps = (Pose * (300 * 16))() if poses else None
    sc = (PoseScore * (300 * 16))()
    for i in range(len(sc)):
        sc[i].n_rows, sc[i].score = 77, 7.0   # garbage the call must clear
    bs = (C.c_int * 300)(*([55] * 300))
    it = (C.c_double * 4)(*intr) if intr is not None else None
    prm = defaults() if p is None else p
    st = VerifyStats()
    st.n_launches = 99
    s = lib().ppf_verify_frame(dets, n_dets, ps, np_ if counts else None, top, depth, rows, cols, it, C.byref(prm) if params else None,
                               sc if scores else None, bs if best else None, C.byref(st))
    return s, sc, bs, st


def _cleared(sc, bs, n_dets, top=4):
    return all(bytes(sc[i]) == bytes(PoseScore()) for i in range(n_dets * top)) and list(bs[:n_dets]) == [-1] * n_dets and \
        sc[n_dets * top].n_rows == 77 and bs[n_dets] == 55   # nothing beyond n_dets touched


def _invalid(r, n_dets=3, top=4, needle=None):
    s, sc, bs, st = r
    assert s == _capi.PPF_ERR_INVALID, (s, _capi.last_error())
    assert "ppf_verify_frame" in _capi.last_error()
    if needle:
        assert needle in _capi.last_error(), _capi.last_error()
    assert st.n_launches == 0 and st.n_host_syncs == 0 and st.n_jobs == 0
    if 0 < n_dets <= 256 and 1 <= top <= 16:
        assert _cleared(sc, bs, n_dets, top)


def test_range_errors():
    dets = _dets(3)
    _invalid(_call(dets, 257), n_dets=257, needle="n_dets")
    _invalid(_call(dets, -1), n_dets=-1, needle="n_dets")
    for top in (0, 17, -3):
        _invalid(_call(dets, 3, top=top), top=top, needle="top")
    _invalid(_call(dets, 3, n_poses=[2, 5, 1]), needle="n_poses[1]")
    _invalid(_call(dets, 3, n_poses=[2, -1, 1]), needle="n_poses[1]")


def test_null_arguments():
    dets = _dets(3)
    _invalid(_call(dets, 3, params=False), needle="params")
    _invalid(_call(dets, 3, poses=False))
    _invalid(_call(dets, 3, counts=False))
    _invalid(_call(None, 3))
    s, sc, bs, st = _call(dets, 3, scores=False)
    assert s == _capi.PPF_ERR_INVALID and list(bs[:3]) == [-1] * 3
    s, sc, bs, st = _call(dets, 3, best=False)
    assert s == _capi.PPF_ERR_INVALID and all(bytes(sc[i]) == bytes(PoseScore()) for i in range(12))
    _invalid(_call(_dets(3, model_cloud=False), 3), needle="detection 0")
    _invalid(_call(_dets(3, scene=False), 3), needle="detection 0")
    bad = _dets(3)
    bad[2].scene = None
    _invalid(_call(bad, 3), needle="detection 2")


def test_parameter_errors():
    dets = _dets(3)
    for field, values in (("inlier_dist", (0.0, -0.001, NAN, INF)), ("normal_cos", (1.5, -1.01, NAN)),
                          ("depth_tol", (0.0, -1.0, NAN, INF)), ("model_step", (0, -2)), ("flags", (4, 8, -1))):
        for v in values:
            p = defaults()
            setattr(p, field, v)
            _invalid(_call(dets, 3, p=p))


def test_depth_image_errors():
    dets = _dets(3)
    img = (C.c_float * 16)()
    for rows, cols in ((0, 4), (4, 0), (-1, 4), (70000, 70000)):
        _invalid(_call(dets, 3, depth=img, rows=rows, cols=cols))
    _invalid(_call(dets, 3, depth=img, rows=4, cols=4, intr=None))
    for bad in ((0.0, 1.0, 2.0, 2.0), (1.0, 0.0, 2.0, 2.0), (NAN, 1.0, 2.0, 2.0), (1.0, INF, 2.0, 2.0), (1.0, 1.0, NAN, 2.0),
                (1.0, 1.0, 2.0, -INF)):
        _invalid(_call(dets, 3, depth=img, rows=4, cols=4, intr=bad))


def test_skipped_detections_need_no_clouds():
    """detections without poses may have NULL clouds; without a depth image intr may be NULL"""
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    s, sc, bs, st = _call((FrameDetection * 4)(), 4, n_poses=[0] * 4, intr=None)
    assert s == _capi.PPF_ERR_HIP and list(bs[:4]) == [-1] * 4


def test_verify_frame_without_a_device_is_loud():
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    img = (C.c_float * 16)()
    for n, kw in ((0, {}), (3, {}), (3, dict(depth=img, rows=4, cols=4))):
        s, sc, bs, st = _call(_dets(n), n, **kw)
        assert s == _capi.PPF_ERR_HIP
        assert "no HIP device" in _capi.last_error() and "ppf_verify_frame" in _capi.last_error()
        assert st.n_launches == 0 and st.n_host_syncs == 0
        if n:
            assert _cleared(sc, bs, n)
