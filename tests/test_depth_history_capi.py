"""ppf_depth_history's C-ABI surface without a GPU: the symbols are exported and bound, the three records as a C++ compiler
lays them out equal their ctypes mirrors, the defaults, every argument error comes before any device work (the handle stays
NULL, the stats zero, t where it was), the ends of every range are accepted, creation fails loudly (PPF_ERR_HIP) when there is
no device, and the demo is C++11 for g++ and clang++."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import DepthHistoryDesc, DepthHistoryParams, DepthHistoryStats, DepthParams, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
PARAM_FIELDS = ["window", "range_abs", "range_quad", "min_support", "max_age", "flags", "reserved"]
STATS_FIELDS = ["n_kept", "n_measured", "n_filled", "n_unsupported", "n_empty", "n_changed", "frame", "n_launches", "n_host_syncs",
                "ms_wall", "reserved"]
DESC_FIELDS = ["rows", "cols", "window", "reserved0", "frames", "device_bytes", "reserved"]
ENTRIES = ["ppf_default_depth_history_params", "ppf_depth_history_create", "ppf_depth_history_push", "ppf_depth_history_push_device",
           "ppf_depth_history_reset", "ppf_depth_history_info", "ppf_depth_history_release"]
HAVE_GPU = lib().ppf_device_count() > 0


def test_symbols_are_exported_and_bound():
    raw = C.CDLL(_capi.LIB_PATH)   # a handle of its own: nothing is bound on it yet
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _capi._SIGNATURES, name
        res, args = _capi._SIGNATURES[name]
        assert list(getattr(lib(), name).argtypes) == list(args) and getattr(lib(), name).restype == res, name


def test_records_match_the_header(tmp_path):
    records = (("ppf_depth_history_params", DepthHistoryParams, PARAM_FIELDS), ("ppf_depth_history_stats", DepthHistoryStats, STATS_FIELDS),
               ("ppf_depth_history_desc", DepthHistoryDesc, DESC_FIELDS))
    consts = ["PPF_HISTORY_MEAN", "PPF_HISTORY_MAX_WINDOW", "PPF_HISTORY_MAX_AGE", "PPF_HISTORY_MEASURED", "PPF_HISTORY_FILLED",
              "PPF_HISTORY_UNSUPPORTED", "PPF_HISTORY_CHANGED", "PPF_ABI_VERSION"]
    expr, got = [], []
    for cname, cls, fields in records:
        expr += [f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields]
        got += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
        assert [f for f, _ in cls._fields_] == fields
    expr += consts
    got += [getattr(_capi, c) for c in consts]
    src = tmp_path / "dhsz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ppf_hip.h"\nint main(){\n' +
                   "".join(f'std::printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "dhsz"
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert want[-8:] == [1, 16, 15, 1, 2, 3, 16, 4]            # the interface only grows: the ABI version stays


def depth_defaults():
    p = DepthParams()
    lib().ppf_default_depth_params(C.byref(p))
    return p


def defaults():
    p = DepthHistoryParams()
    p.window, p.range_abs, p.range_quad, p.min_support, p.max_age, p.flags = 9, 9.0, 9.0, 9, 9, 9
    for i in range(4):
        p.reserved[i] = 9
    lib().ppf_default_depth_history_params(C.byref(p))
    return p


def test_defaults():
    p = defaults()
    assert (p.window, p.range_abs, p.range_quad, p.min_support, p.max_age, p.flags) == (8, float(np.float32(0.01)), 0.0, 1, 7, 0)
    assert list(p.reserved) == [0, 0, 0, 0]
    lib().ppf_default_depth_history_params(None)   # no crash


def hparams(**kw):
    p = defaults()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def dparams(**kw):
    p = depth_defaults()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def create(rows=4, cols=6, dp=None, hp=None, out=True):
    dprm = depth_defaults() if dp is None else dp
    hprm = defaults() if hp is None else hp
    h = C.c_void_p(0x5A5A)
    s = lib().ppf_depth_history_create(rows, cols, C.byref(dprm) if dprm is not False else None, C.byref(hprm) if hprm is not False else None,
                                       C.byref(h) if out else None)
    return s, h


CREATE_ERRORS = [
    ("NULL history params", dict(hp=False)),
    ("NULL depth params", dict(dp=False)),
    ("window 0", dict(hp=hparams(window=0))),
    ("window 17", dict(hp=hparams(window=17, min_support=1))),
    ("range_abs 0", dict(hp=hparams(range_abs=0.0))),
    ("range_abs < 0", dict(hp=hparams(range_abs=-0.01))),
    ("range_abs nan", dict(hp=hparams(range_abs=math.nan))),
    ("range_abs inf", dict(hp=hparams(range_abs=math.inf))),
    ("range_quad < 0", dict(hp=hparams(range_quad=-1.0))),
    ("range_quad nan", dict(hp=hparams(range_quad=math.nan))),
    ("range_quad inf", dict(hp=hparams(range_quad=math.inf))),
    ("min_support 0", dict(hp=hparams(min_support=0))),
    ("min_support window + 1", dict(hp=hparams(window=5, min_support=6))),
    ("max_age -1", dict(hp=hparams(max_age=-1))),
    ("max_age 16", dict(hp=hparams(max_age=16))),
    ("flags 2", dict(hp=hparams(flags=2))),
    ("rows 0", dict(rows=0)),
    ("cols -1", dict(cols=-1)),
    ("rows * cols > INT32_MAX", dict(rows=65536, cols=32768)),
    ("format 2", dict(dp=dparams(format=2))),
    ("u16 scale 0", dict(dp=dparams(format=_capi.PPF_DEPTH_U16, depth_scale=0.0))),
    ("u16 scale nan", dict(dp=dparams(format=_capi.PPF_DEPTH_U16, depth_scale=math.nan))),
    ("z_min inf", dict(dp=dparams(z_min=math.inf))),
    ("z_max nan", dict(dp=dparams(z_max=math.nan))),
    ("z_max < 0", dict(dp=dparams(z_max=-1.0))),
]


@pytest.mark.parametrize("name,kw", CREATE_ERRORS, ids=[c[0] for c in CREATE_ERRORS])
def test_create_argument_errors_precede_any_device_work(name, kw):
    s, h = create(**kw)
    assert s == _capi.PPF_ERR_INVALID, (name, _capi.last_error())
    assert h.value is None, name                                  # *out is NULL on every error
    assert "ppf_depth_history_create:" in _capi.last_error()


def test_create_out_null_and_handle_nulls():
    s, _ = create(out=False)
    assert s == _capi.PPF_ERR_INVALID and "out is NULL" in _capi.last_error()
    assert lib().ppf_depth_history_reset(None) == _capi.PPF_ERR_INVALID
    d = DepthHistoryDesc()
    C.memset(C.byref(d), 0x5A, C.sizeof(d))
    assert lib().ppf_depth_history_info(None, C.byref(d)) == _capi.PPF_ERR_INVALID and bytes(d) == bytes(C.sizeof(d))
    assert lib().ppf_depth_history_release(None) == _capi.PPF_OK   # as free(NULL)
    img, out = np.ones((4, 6), np.float32), np.full((4, 6), np.float32(7.0))
    for entry, extra in ((lib().ppf_depth_history_push, ()), (lib().ppf_depth_history_push_device, (None,))):
        st = DepthHistoryStats()
        C.memset(C.byref(st), 0x5A, C.sizeof(st))
        s = entry(None, C.c_void_p(img.ctypes.data), 0, C.c_void_p(out.ctypes.data), None, *extra, C.byref(st))
        assert s == _capi.PPF_ERR_INVALID and bytes(st) == bytes(C.sizeof(st)) and "history is NULL" in _capi.last_error()
        assert entry(None, C.c_void_p(img.ctypes.data), 0, C.c_void_p(out.ctypes.data), None, *extra, None) == _capi.PPF_ERR_INVALID
    assert (out == 7.0).all()


def test_depth_flags_are_ignored_and_range_ends_reach_the_device_check():
    """the ends of every range pass the argument checks: the status is PPF_OK with a device and PPF_ERR_HIP without"""
    cases = [dict(dp=dparams(flags=_capi.PPF_DEPTH_FP64)), dict(dp=dparams(flags=6)),
             dict(hp=hparams(window=1, min_support=1)), dict(hp=hparams(window=16, min_support=16)), dict(hp=hparams(max_age=0)),
             dict(hp=hparams(max_age=15)), dict(hp=hparams(flags=_capi.PPF_HISTORY_MEAN)),
             dict(hp=hparams(range_abs=float(np.finfo(np.float32).tiny), range_quad=0.0)), dict(rows=1, cols=1)]
    for kw in cases:
        s, h = create(**kw)
        if HAVE_GPU:
            assert s == _capi.PPF_OK and h.value, (kw, _capi.last_error())
            assert lib().ppf_depth_history_release(h) == _capi.PPF_OK
        else:
            assert s == _capi.PPF_ERR_HIP and h.value is None, (kw, _capi.last_error())


def test_without_a_device_it_is_loud():
    s, h = create()
    if HAVE_GPU:
        assert s == _capi.PPF_OK
        lib().ppf_depth_history_release(h)
        return
    assert s == _capi.PPF_ERR_HIP and h.value is None
    assert "no HIP device" in _capi.last_error() and "ppf_depth_history_create" in _capi.last_error()
    from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DepthHistory
    for call in (lambda: DepthHistory((4, 6)), lambda: CloudProcessor(None, None).FuseDepth(np.ones((4, 6), np.float32))):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_HIP


def build_demo(tmp_path, compiler="g++"):
    exe = str(tmp_path / f"depth_history_demo_{compiler}")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "depth_history_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_demo_compiles_as_cxx11(tmp_path, compiler):
    build_demo(tmp_path, compiler)


def test_demo_fails_loudly_without_gpu(tmp_path):
    exe = build_demo(tmp_path)
    if HAVE_GPU:
        return
    (tmp_path / "d.f32").write_bytes(np.ones((4, 6), np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "d.f32"), "4", "6", "500", "500", "3", "2"], capture_output=True, text=True)
    assert r.returncode == 10 + _capi.PPF_ERR_HIP, (r.returncode, r.stderr)
    assert "ppf_depth_history_create" in r.stderr


def test_python_wrapper_rejects_unknown_keys_and_other_dtypes():
    from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DepthHistory
    for call in (lambda: DepthHistory((4, 6), params=dict(windw=3)), lambda: DepthHistory((4, 6), dtype=np.float64),
                 lambda: DepthHistory((2, 4, 6)), lambda: DepthHistory((4, 6), params=dict(window=17)),
                 lambda: DepthHistory((4, 6), z_max=-1.0), lambda: CloudProcessor(None, None).FuseDepth(None),
                 lambda: CloudProcessor(None, None).FuseDepth(np.ones((4, 6), np.float32), params=dict(max_agee=3)),
                 lambda: CloudProcessor(None, None).FuseDepth(np.ones((4, 6), np.float64))):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID
    with pytest.raises(_capi.PPFError) as e:
        DepthHistory((4, 6), params=dict(window=4, min_support=5))
    assert e.value.status == _capi.PPF_ERR_INVALID and "min_support" in str(e.value)
