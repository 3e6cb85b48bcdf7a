"""The C-ABI surface of ppf_prep_regions without a GPU: the symbols are exported and bound, ppf_region_params as a C compiler lays
it out equals its ctypes mirror, the defaults (and the oracle's), every argument error comes before any device work with the
outputs cleared, the entry fails loudly (PPF_ERR_HIP) when there is no device, the Python wrappers reject a misspelt parameter,
and examples/region_demo.cpp compiles as C++11."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import region_oracle as R
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import ClusterInfo, ClusterStats, RegionParams, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
SENTINEL = 0x5A5A5A5A
FAKE = C.c_void_p(0x1000)   # a cloud handle that no argument check may follow


def test_symbols_are_exported_and_bound():
    for name in ("ppf_default_region_params", "ppf_prep_regions", "ppf_cloud_set_curvature"):
        assert name in _capi._SIGNATURES and getattr(lib(), name) is not None
    header = open(os.path.join(ROOT, "include", "ppf_hip.h")).read()
    assert "#define PPF_ABI_VERSION 4 " in header and "ppf_status ppf_prep_regions(" in header


def test_struct_layout_matches_the_header(tmp_path):
    expr, got = ["sizeof(ppf_region_params)"], [C.sizeof(RegionParams)]
    for f, _ in RegionParams._fields_:
        expr.append(f"offsetof(ppf_region_params, {f})")
        got.append(getattr(RegionParams, f).offset)
    expr += ["PPF_REGION_UNORIENTED", "PPF_CLUSTER_MAX_CLUSTERS"]
    got += [_capi.PPF_REGION_UNORIENTED, _capi.PPF_CLUSTER_MAX_CLUSTERS]
    src = tmp_path / "rsz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ppf_hip.h"\nint main(){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "rsz"
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want and C.sizeof(RegionParams) == 44
    assert R.INFO.itemsize == C.sizeof(ClusterInfo) and R.UNORIENTED == _capi.PPF_REGION_UNORIENTED


def defaults():
    p = RegionParams()
    lib().ppf_default_region_params(C.byref(p))
    return p


def test_defaults():
    p = RegionParams()
    for f, _ in RegionParams._fields_[:-1]:
        setattr(p, f, 7)
    p.reserved[2] = 7
    lib().ppf_default_region_params(C.byref(p))
    assert (p.tolerance, p.normal_cos, p.curvature_threshold, p.min_size, p.max_size, p.max_regions, p.flags) == \
        (np.float32(0.01), np.float32(0.9659258), np.float32(0.03), 100, 0, 64, 0) and list(p.reserved) == [0] * 4
    assert p.normal_cos == np.float32(math.cos(math.radians(15.0)))
    lib().ppf_default_region_params(None)   # no crash
    d = R.DEFAULTS
    assert (np.float32(d["tolerance"]), np.float32(d["normal_cos"]), np.float32(d["curvature_threshold"]), d["min_size"], d["max_size"],
            d["max_regions"], d["flags"]) == (p.tolerance, p.normal_cos, p.curvature_threshold, 100, 0, 64, 0)


BAD_PARAMS = [("tolerance 0", dict(tolerance=0.0)), ("tolerance < 0", dict(tolerance=-0.01)), ("tolerance nan", dict(tolerance=math.nan)),
              ("tolerance inf", dict(tolerance=math.inf)), ("cos < -1", dict(normal_cos=-1.0000001)), ("cos > 1", dict(normal_cos=1.0000001)),
              ("cos nan", dict(normal_cos=math.nan)), ("cos inf", dict(normal_cos=math.inf)), ("curvature < 0", dict(curvature_threshold=-0.001)),
              ("curvature nan", dict(curvature_threshold=math.nan)), ("min_size 0", dict(min_size=0)), ("max_size < 0", dict(max_size=-1)),
              ("no regions", dict(max_regions=0)), ("too many regions", dict(max_regions=257)), ("unknown flag", dict(flags=2)),
              ("negative flags", dict(flags=-1))]


def call_regions(ins, n, prm, outs=True, info=True, counts=True, labels=None):
    """one ppf_prep_regions call on handles that must not be followed; returns (status, out handles, info bytes, counts, stats)"""
    k = max(n, 1) if 0 <= n <= 256 else 1
    mr = min(max(prm.max_regions, 1), 256) if prm is not None else 1
    out = (C.c_void_p * (k * mr))(*([SENTINEL] * (k * mr)))
    rows = (ClusterInfo * (k * mr))()
    C.memset(rows, 0x5A, C.sizeof(rows))
    cnt = (C.c_int32 * (k * 4))(*([7] * (k * 4)))
    st = ClusterStats()
    st.n_launches = 7
    s = lib().ppf_prep_regions(ins, n, C.byref(prm) if prm is not None else None, None, 0, 0, out if outs else None, rows if info else None,
                               cnt if counts else None, labels, C.byref(st))
    return s, list(out), bytes(rows), list(cnt), st


@pytest.mark.parametrize("name,kw", BAD_PARAMS, ids=[c[0] for c in BAD_PARAMS])
def test_a_parameter_out_of_range_is_an_argument_error(name, kw):
    p = defaults()
    for k, v in kw.items():
        setattr(p, k, v)
    s, out, rows, cnt, st = call_regions((C.c_void_p * 2)(FAKE, FAKE), 2, p)
    assert s == _capi.PPF_ERR_INVALID and "ppf_prep_regions" in _capi.last_error(), name
    assert out == [None] * len(out) and rows == bytes(len(rows)) and cnt == [0] * 8 and st.n_launches == 0


def test_the_edges_of_the_ranges_are_taken():
    """-1, 1, 0 and +inf pass the parameter check: the call goes on to the next check, a NULL cloud"""
    for kw in (dict(normal_cos=-1.0), dict(normal_cos=1.0), dict(curvature_threshold=0.0), dict(curvature_threshold=math.inf),
               dict(max_regions=1), dict(max_regions=256), dict(flags=_capi.PPF_REGION_UNORIENTED)):
        p = defaults()
        for k, v in kw.items():
            setattr(p, k, v)
        s = call_regions((C.c_void_p * 2)(FAKE, None), 2, p)[0]
        assert s == _capi.PPF_ERR_INVALID and "in[1] is NULL" in _capi.last_error(), kw


def test_argument_errors_precede_any_device_work():
    p = defaults()
    ins = (C.c_void_p * 2)(FAKE, FAKE)
    for n in (-1, 257):
        s = call_regions(ins, n, p)[0]
        assert s == _capi.PPF_ERR_INVALID and "n_clouds" in _capi.last_error()
    for kw in (dict(ins=None), dict(prm=None)):
        s, out, rows, cnt, st = call_regions(kw.get("ins", ins), 2, kw.get("prm", p))
        assert s == _capi.PPF_ERR_INVALID and out == [None] * len(out) and rows == bytes(len(rows)) and cnt == [0] * 8
    assert call_regions(ins, 2, p, outs=False)[0] == _capi.PPF_ERR_INVALID
    assert call_regions(ins, 2, p, info=False)[0] == _capi.PPF_ERR_INVALID
    assert call_regions(ins, 2, p, counts=False)[0] == _capi.PPF_ERR_INVALID
    s, out, rows, cnt, st = call_regions((C.c_void_p * 2)(FAKE, None), 2, p)
    assert s == _capi.PPF_ERR_INVALID and "in[1]" in _capi.last_error() and out == [None] * 128 and cnt == [0] * 8
    assert st.n_launches == 0 and st.n_clouds == 0
    # the intrinsics, when given, are checked too
    out, rows, cnt = (C.c_void_p * 128)(), (ClusterInfo * 128)(), (C.c_int32 * 8)()
    bad = (C.c_double * 4)(400.0, math.nan, 1.0, 1.0)
    assert lib().ppf_prep_regions(ins, 2, C.byref(p), bad, 10, 10, out, rows, cnt, None, None) == _capi.PPF_ERR_INVALID   # stats may be NULL
    ok = (C.c_double * 4)(400.0, 400.0, 1.0, 1.0)
    assert lib().ppf_prep_regions(ins, 2, C.byref(p), ok, 0, 10, out, rows, cnt, None, None) == _capi.PPF_ERR_INVALID
    # ppf_cloud_set_curvature
    assert lib().ppf_cloud_set_curvature(None, (C.c_float * 1)(), 1) == _capi.PPF_ERR_INVALID


def test_without_a_device_the_entry_is_loud():
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    p = defaults()
    s, out, rows, cnt, st = call_regions((C.c_void_p * 2)(FAKE, FAKE), 2, p)
    assert s == _capi.PPF_ERR_HIP and "no HIP device" in _capi.last_error() and "ppf_prep_regions" in _capi.last_error()
    assert out == [None] * len(out) and rows == bytes(len(rows)) and cnt == [0] * 8 and st.n_launches == 0
    from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor
    with pytest.raises(_capi.PPFError) as e:
        CloudProcessor(np.zeros((10, 3), np.float32), np.zeros((4, 4), np.float32)).ProposeRegions(np.eye(3))
    assert e.value.status == _capi.PPF_ERR_HIP
    with pytest.raises(_capi.PPFError) as e:
        CloudProcessor().ProposeRegions(np.eye(3))
    assert e.value.status == _capi.PPF_ERR_INVALID


def test_python_wrapper_rejects_a_misspelt_parameter():
    from yolo_ppf_pose_estimation_amd.cloud_processor import _params, region_clouds

    def _region_params(params):
        return _params(RegionParams, "ppf_default_region_params", params, "region")
    assert _region_params(dict(max_regions=7, flags=1)).max_regions == 7 and _region_params(None).max_regions == 64
    for call in (lambda: _region_params(dict(max_clusters=7)), lambda: region_clouds([], dict(normal_cosine=0.5))):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID and "unknown region parameter" in str(e.value)


def build_demo(tmp_path, compiler="g++"):
    exe = str(tmp_path / f"region_demo_{compiler}")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "region_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_region_demo_compiles_as_cxx11(tmp_path, compiler):
    build_demo(tmp_path, compiler)


def test_region_demo_fails_loudly_without_gpu(tmp_path):
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    exe = build_demo(tmp_path)
    (tmp_path / "depth.f32").write_bytes(np.ones((8, 8), np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "depth.f32"), "8", "8", "400", "400", "4", "4"], capture_output=True, text=True)
    assert r.returncode == 10 + _capi.PPF_ERR_HIP, (r.returncode, r.stderr)
    assert "no HIP device" in r.stderr
