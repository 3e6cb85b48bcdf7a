"""The C-ABI surface of the plane removal without a GPU: ppf_plane_params, ppf_plane_info and ppf_plane_stats as a C compiler
lays them out equal their ctypes and numpy mirrors, the defaults, every argument error of ppf_prep_planes and
ppf_prep_planes_apply comes before any device work with the outputs cleared, the entries fail loudly (PPF_ERR_HIP) when
there is no device, and examples/plane_remove_demo.cpp compiles as C++11."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import plane_oracle as O
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import PlaneInfo, PlaneParams, PlaneStats, lib
from yolo_ppf_pose_estimation_amd.cloud_processor import PLANE_INFO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
SENTINEL = 0x5A5A5A5A
FAKE = C.c_void_p(0x1000)   # a cloud handle that no argument check may follow


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"ppf_plane_params": PlaneParams, "ppf_plane_info": PlaneInfo, "ppf_plane_stats": PlaneStats}
    expr, got = [], []
    for name, cls in structs.items():
        expr.append(f"sizeof({name})")
        got.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            expr.append(f"offsetof({name}, {f})")
            got.append(getattr(cls, f).offset)
    consts = ["PPF_PLANE_NONE", "PPF_PLANE_REMOVED", "PPF_PLANE_REJECTED", "PPF_PLANE_NO_REFIT", "PPF_PLANE_REMOVE_BEHIND",
              "PPF_PLANE_MAX_PLANES", "PPF_PLANE_MAX_HYPOTHESES"]
    expr += consts
    got += [getattr(_capi, c) for c in consts]
    src = tmp_path / "psz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppf_hip.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "psz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    # the numpy records of the wrapper and of the oracle are the same 64 bytes
    for dt in (PLANE_INFO, O.INFO):
        assert dt.itemsize == C.sizeof(PlaneInfo) == 64
        assert [dt.fields[f][1] for f, _ in PlaneInfo._fields_] == [getattr(PlaneInfo, f).offset for f, _ in PlaneInfo._fields_]
    assert (O.NONE, O.REMOVED, O.REJECTED, O.NO_REFIT, O.REMOVE_BEHIND) == (0, 1, 2, 1, 2)


def defaults():
    p = PlaneParams()
    lib().ppf_default_plane_params(C.byref(p))
    return p


def test_defaults():
    p = PlaneParams()
    for f, _ in PlaneParams._fields_[:-1]:
        setattr(p, f, 7)
    p.reserved[2] = 7
    lib().ppf_default_plane_params(C.byref(p))
    assert (p.distance_threshold, p.n_hypotheses, p.seed, p.max_planes, p.min_inliers, p.min_inlier_share, p.flags) == \
        (np.float32(0.005), 256, 1, 1, 100, np.float32(0.10), 0) and list(p.reserved) == [0] * 4
    lib().ppf_default_plane_params(None)   # no crash
    d = O.DEFAULTS
    assert (np.float32(d["distance_threshold"]), d["n_hypotheses"], d["seed"], d["max_planes"], d["min_inliers"],
            np.float32(d["min_inlier_share"]), d["flags"]) == (p.distance_threshold, 256, 1, 1, 100, p.min_inlier_share, 0)


BAD_PARAMS = [("threshold 0", dict(distance_threshold=0.0)), ("threshold < 0", dict(distance_threshold=-0.01)),
              ("threshold nan", dict(distance_threshold=math.nan)), ("threshold inf", dict(distance_threshold=math.inf)),
              ("no hypotheses", dict(n_hypotheses=0)), ("too many hypotheses", dict(n_hypotheses=4097)), ("no planes", dict(max_planes=0)),
              ("too many planes", dict(max_planes=5)), ("min_inliers 2", dict(min_inliers=2)), ("share < 0", dict(min_inlier_share=-0.1)),
              ("share > 1", dict(min_inlier_share=1.5)), ("share nan", dict(min_inlier_share=math.nan)), ("unknown flag", dict(flags=4)),
              ("negative flags", dict(flags=-1))]


def call_planes(ins, n, prm, outs=True, info=True, labels=None):
    """one ppf_prep_planes call on handles that must not be followed; returns (status, out handles, info bytes, stats)"""
    k = max(n, 1) if 0 <= n <= 256 else 1
    out = (C.c_void_p * k)(*([SENTINEL] * k))
    rows = (PlaneInfo * (k * 4))()
    C.memset(rows, 0x5A, C.sizeof(rows))
    st = PlaneStats()
    st.n_launches = 7
    s = lib().ppf_prep_planes(ins, n, C.byref(prm) if prm is not None else None, out if outs else None, rows if info else None, labels, C.byref(st))
    return s, list(out), bytes(rows), st


@pytest.mark.parametrize("name,kw", BAD_PARAMS, ids=[c[0] for c in BAD_PARAMS])
def test_a_parameter_out_of_range_is_an_argument_error(name, kw):
    p = defaults()
    for k, v in kw.items():
        setattr(p, k, v)
    ins = (C.c_void_p * 2)(FAKE, FAKE)
    s, out, rows, st = call_planes(ins, 2, p)
    assert s == _capi.PPF_ERR_INVALID and "ppf_prep_planes" in _capi.last_error(), name
    planes = min(max(p.max_planes, 1), 4)
    assert out == [None, None] and rows[:2 * planes * 64] == bytes(2 * planes * 64) and st.n_launches == 0
    o = C.c_void_p(SENTINEL)
    info = (PlaneInfo * 1)()
    assert lib().ppf_prep_planes_apply(FAKE, info, 1, C.byref(p), C.byref(o)) == _capi.PPF_ERR_INVALID
    assert o.value is None and "ppf_prep_planes_apply" in _capi.last_error()


def test_argument_errors_precede_any_device_work():
    p = defaults()
    ins = (C.c_void_p * 2)(FAKE, FAKE)
    for n in (-1, 257):
        s, out, rows, _ = call_planes(ins, n, p)
        assert s == _capi.PPF_ERR_INVALID and "n_clouds" in _capi.last_error()
    s, out, rows, st = call_planes(None, 2, p)
    assert s == _capi.PPF_ERR_INVALID and out == [None, None] and rows[:128] == bytes(128)
    s, out, rows, st = call_planes(ins, 2, None)
    assert s == _capi.PPF_ERR_INVALID and out == [None, None] and rows[:128] == bytes(128)
    assert call_planes(ins, 2, p, outs=False)[0] == _capi.PPF_ERR_INVALID
    s, out, _, _ = call_planes(ins, 2, p, info=False)
    assert s == _capi.PPF_ERR_INVALID and out == [None, None]
    s, out, rows, st = call_planes((C.c_void_p * 2)(FAKE, None), 2, p)
    assert s == _capi.PPF_ERR_INVALID and "in[1]" in _capi.last_error() and out == [None, None] and rows[:128] == bytes(128)
    assert st.n_launches == 0 and st.n_clouds == 0
    assert lib().ppf_prep_planes(ins, -1, C.byref(p), (C.c_void_p * 2)(), (PlaneInfo * 2)(), None, None) == _capi.PPF_ERR_INVALID   # stats may be NULL
    # apply
    info = (PlaneInfo * 4)()
    o = C.c_void_p(SENTINEL)
    ap = lib().ppf_prep_planes_apply
    for args in ((None, info, 1, C.byref(p)), (FAKE, info, -1, C.byref(p)), (FAKE, info, 5, C.byref(p)), (FAKE, None, 1, C.byref(p)),
                 (FAKE, info, 1, None)):
        o.value = SENTINEL
        assert ap(*args, C.byref(o)) == _capi.PPF_ERR_INVALID and o.value is None and "ppf_prep_planes_apply" in _capi.last_error()
    assert ap(FAKE, info, 1, C.byref(p), None) == _capi.PPF_ERR_INVALID
    info[0].status = _capi.PPF_PLANE_REMOVED
    info[0].n[0] = math.nan
    assert ap(FAKE, info, 1, C.byref(p), C.byref(o)) == _capi.PPF_ERR_INVALID and "not finite" in _capi.last_error()


def test_without_a_device_the_entries_are_loud():
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    p = defaults()
    s, out, rows, st = call_planes((C.c_void_p * 2)(FAKE, FAKE), 2, p)
    assert s == _capi.PPF_ERR_HIP and "no HIP device" in _capi.last_error() and "ppf_prep_planes" in _capi.last_error()
    assert out == [None, None] and rows[:128] == bytes(128) and st.n_launches == 0
    o = C.c_void_p(SENTINEL)
    assert lib().ppf_prep_planes_apply(FAKE, None, 0, C.byref(p), C.byref(o)) == _capi.PPF_ERR_HIP and o.value is None
    from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor
    with pytest.raises(_capi.PPFError) as e:
        CloudProcessor(np.zeros((10, 3), np.float32)).RemovePlanes()
    assert e.value.status == _capi.PPF_ERR_HIP
    with pytest.raises(_capi.PPFError) as e:
        CloudProcessor().RemovePlanes()
    assert e.value.status == _capi.PPF_ERR_INVALID


def test_python_wrapper_rejects_a_misspelt_parameter():
    from yolo_ppf_pose_estimation_amd.cloud_processor import _params, cluster_clouds, filter_depth, remove_planes, segment_depth

    def _plane_params(params):
        return _params(PlaneParams, "ppf_default_plane_params", params, "plane")
    assert _plane_params(dict(n_hypotheses=64, seed=3)).n_hypotheses == 64 and _plane_params(None).n_hypotheses == 256
    for call in (lambda: _plane_params(dict(n_hypothesis=64)), lambda: remove_planes([], dict(max_plane=2))):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID and "unknown plane parameter" in str(e.value)
    img = np.zeros((2, 2), np.float32)
    for what, call in (("cluster", lambda: cluster_clouds([], dict(max_cluster=2))), ("depth filter", lambda: filter_depth(img, params=dict(radios=2))),
                       ("segment", lambda: segment_depth(img, params=dict(max_segment=2)))):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID and f"unknown {what} parameter" in str(e.value)


def build_demo(tmp_path, compiler="g++"):
    exe = str(tmp_path / f"plane_remove_demo_{compiler}")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "plane_remove_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe],
                   check=True)
    return exe


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_plane_remove_demo_compiles_as_cxx11(tmp_path, compiler):
    build_demo(tmp_path, compiler)


def test_plane_remove_demo_fails_loudly_without_gpu(tmp_path):
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    exe = build_demo(tmp_path)
    (tmp_path / "scene.f32").write_bytes(np.zeros((10, 3), np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "scene.f32"), "10"], capture_output=True, text=True)
    assert r.returncode == 10 + _capi.PPF_ERR_HIP, (r.returncode, r.stderr)
    assert "no HIP device" in r.stderr
