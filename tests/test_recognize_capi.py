"""ppf_recognizer_* / ppf_recognize_frame's C-ABI surface without a GPU: the symbols are exported and bound, the records as a
C++ compiler lays them out equal their ctypes mirrors, the defaults, every argument error comes before any device work and
leaves the outputs zero, the ends of every range are accepted up to the point where a device is needed, the calls fail loudly
(PPF_ERR_HIP) when there is no device, and the demo is C++11 for g++ and clang++.

A recogniser only exists where there is a device.  Without one the calls get a handle that is never looked into (every check
in front of the device check reads the arguments alone); with one they get a real recogniser of one small model."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import RecognizeParams, RecognizerInfo, RecognizeScore, RecognizeStats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
INFO_FIELDS = ["n_rows", "n_bins", "in_lds", "n_keys", "bytes", "reserved"]
PARAM_FIELDS = ["max_rows", "top", "min_score", "min_precision", "flags", "reserved"]
SCORE_FIELDS = ["model", "reserved", "n_known", "n_keys_hit", "precision", "recall", "score"]
STATS_FIELDS = ["n_clouds", "n_models", "n_launches", "n_host_syncs", "ms_wall", "reserved"]
ENTRIES = ["ppf_recognizer_create", "ppf_recognizer_retain", "ppf_recognizer_release", "ppf_recognizer_model_info", "ppf_recognizer_keys",
           "ppf_default_recognize_params", "ppf_recognize_frame"]
HAVE_GPU = lib().ppf_device_count() > 0


def test_symbols_are_exported_and_bound():
    raw = C.CDLL(_capi.LIB_PATH)   # a handle of its own: nothing is bound on it yet
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _capi._SIGNATURES, name
        res, args = _capi._SIGNATURES[name]
        assert list(getattr(lib(), name).argtypes) == list(args) and getattr(lib(), name).restype == res, name


def test_records_match_the_header(tmp_path):
    from yolo_ppf_pose_estimation_amd.cloud_processor import RECOGNIZE_SCORE
    src = tmp_path / "rcsz.cpp"
    records = (("ppf_recognizer_info", INFO_FIELDS, RecognizerInfo), ("ppf_recognize_params", PARAM_FIELDS, RecognizeParams),
               ("ppf_recognize_score", SCORE_FIELDS, RecognizeScore), ("ppf_recognize_stats", STATS_FIELDS, RecognizeStats))
    expr = []
    for name, fields, _ in records:
        expr += [f"sizeof({name})"] + [f"offsetof({name}, {f})" for f in fields]
    expr += ["PPF_RECOGNIZE_MAX_MODELS", "PPF_RECOGNIZE_MAX_CLOUDS", "PPF_RECOGNIZE_MAX_ROWS", "PPF_RECOGNIZE_MAX_TOP", "PPF_ABI_VERSION"]
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ppf_hip.h"\nint main(){\n' +
                   "".join(f'std::printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "rcsz"
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    got = []
    for _, fields, cls in records:
        got += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
        assert [f for f, _ in cls._fields_] == fields
    got += [_capi.PPF_RECOGNIZE_MAX_MODELS, _capi.PPF_RECOGNIZE_MAX_CLOUDS, _capi.PPF_RECOGNIZE_MAX_ROWS, _capi.PPF_RECOGNIZE_MAX_TOP,
            _capi.PPF_ABI_VERSION]
    assert got == want
    assert want[-5:] == [64, 256, 2048, 16, 4]       # the interface only grows: the ABI version stays
    assert RECOGNIZE_SCORE.itemsize == C.sizeof(RecognizeScore) and list(RECOGNIZE_SCORE.names) == SCORE_FIELDS
    assert [RECOGNIZE_SCORE.fields[f][1] for f in SCORE_FIELDS] == [getattr(RecognizeScore, f).offset for f in SCORE_FIELDS]


def defaults():
    p = RecognizeParams()
    C.memset(C.byref(p), 0x5A, C.sizeof(p))
    lib().ppf_default_recognize_params(C.byref(p))
    return p


def rparams(**kw):
    p = defaults()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults():
    p = defaults()
    assert (p.max_rows, p.top, p.min_score, p.min_precision, p.flags) == (512, 2, 0.0, 0.0, 0) and list(p.reserved) == [0, 0, 0, 0]
    lib().ppf_default_recognize_params(None)   # no crash


@pytest.fixture(scope="module")
def handle():
    """(recogniser handle, its model count): a real one where there is a device, else one that must never be looked into"""
    if not HAVE_GPU:
        yield C.c_void_p(0x10), 1
        return
    from yolo_ppf_pose_estimation_amd import synth
    from yolo_ppf_pose_estimation_amd.cloud_processor import Recognizer
    from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
    rec = Recognizer([PPF3DDetector(0.05, 0.05).trainModel(synth.make_solid("torus", n_points=150), presampled=True)])
    yield rec._ptr, 1
    del rec


class Outputs:
    """dirty outputs: an error must clear them"""

    def __init__(self, n_clouds=3, top=16, n_models=1):
        self.n = max(n_clouds, 1)
        self.n_used = (C.c_int32 * self.n)(*([9] * self.n))
        self.counts = (C.c_uint64 * (self.n * n_models * 2))(*([9] * (self.n * n_models * 2)))
        self.ranked = (RecognizeScore * (self.n * top))()
        C.memset(self.ranked, 0x5A, C.sizeof(self.ranked))
        self.n_ranked = (C.c_int32 * self.n)(*([9] * self.n))
        self.st = RecognizeStats()
        C.memset(C.byref(self.st), 0x5A, C.sizeof(self.st))

    def cleared(self, n_clouds, top=None, counts=True):
        """what the arguments size is zero, and nothing behind it is touched"""
        ok = bytes(self.st) == bytes(C.sizeof(self.st))
        ok = ok and list(self.n_used)[:n_clouds] == [0] * n_clouds and list(self.n_ranked)[:n_clouds] == [0] * n_clouds
        if counts and HAVE_GPU:   # counts is sized by the recogniser: it is only passed where the handle is a real one
            ok = ok and not any(self.counts)
        if top is not None:
            cut = n_clouds * top * C.sizeof(RecognizeScore)
            ok = ok and bytes(self.ranked)[:cut] == bytes(cut) and set(bytes(self.ranked)[cut:]) <= {0x5A}
        return ok


def frame_call(handle, n_clouds=3, prm=None, rec=True, clouds=True, ranked=True, n_ranked=True, counts=True):
    ptr, n_models = handle
    p = defaults() if prm is None else prm
    o = Outputs(n_clouds if 0 < n_clouds <= 256 else 3, n_models=n_models)
    arr = (C.c_void_p * max(n_clouds, 1))()   # NULL clouds: allowed, they have no candidates
    s = lib().ppf_recognize_frame(ptr if rec else None, arr if clouds else None, n_clouds, C.byref(p) if p is not False else None, o.n_used,
                                  o.counts if counts and rec and HAVE_GPU else None, o.ranked if ranked else None, o.n_ranked if n_ranked else None, C.byref(o.st))
    return s, o


def test_argument_errors_come_first_and_clear_the_outputs(handle):
    cases = [("NULL recogniser", dict(rec=False), 2), ("NULL params", dict(prm=False), None), ("NULL ranked", dict(ranked=False), None),
             ("NULL n_ranked", dict(n_ranked=False), 2), ("NULL clouds", dict(clouds=False), 2),
             ("max_rows 1", dict(prm=rparams(max_rows=1)), 2), ("max_rows 2049", dict(prm=rparams(max_rows=2049)), 2),
             ("top 0", dict(prm=rparams(top=0)), None), ("top 17", dict(prm=rparams(top=17)), None),
             ("min_score < 0", dict(prm=rparams(min_score=-1e-9)), 2), ("min_score NaN", dict(prm=rparams(min_score=math.nan)), 2),
             ("min_score inf", dict(prm=rparams(min_score=math.inf)), 2), ("min_precision < 0", dict(prm=rparams(min_precision=-1.0)), 2),
             ("min_precision NaN", dict(prm=rparams(min_precision=math.nan)), 2), ("min_precision inf", dict(prm=rparams(min_precision=math.inf)), 2),
             ("unknown flag", dict(prm=rparams(flags=1)), 2)]
    for what, kw, top in cases:
        s, o = frame_call(handle, **kw)
        assert s == _capi.PPF_ERR_INVALID, (what, s, _capi.last_error())
        assert "ppf_recognize_frame" in _capi.last_error(), what
        if kw.get("n_ranked") is False:
            assert list(o.n_used) == [0, 0, 0] and bytes(o.st) == bytes(C.sizeof(o.st)), what
        else:
            assert o.cleared(3, top=top if kw.get("ranked", True) else None, counts=kw.get("rec", True)), what
    for n in (-1, 257):   # a count outside its range sizes nothing: only the stats can be cleared
        s, o = frame_call(handle, n_clouds=n)
        assert s == _capi.PPF_ERR_INVALID and "n_clouds" in _capi.last_error() and bytes(o.st) == bytes(C.sizeof(o.st))
        assert list(o.n_used) == [9, 9, 9]


def test_range_edges_reach_the_device_check(handle):
    for kw in (dict(max_rows=2), dict(max_rows=2048), dict(top=1), dict(top=16), dict(min_score=0.0), dict(min_score=1e300),
               dict(min_precision=0.0), dict(min_precision=1.0)):
        s, o = frame_call(handle, prm=rparams(**kw))
        if HAVE_GPU:
            assert s == _capi.PPF_OK and (o.st.n_clouds, o.st.n_models, o.st.n_host_syncs, o.st.n_launches) == (3, 1, 1, 2), (kw, _capi.last_error())
            assert list(o.n_ranked) == [0, 0, 0] and list(o.n_used) == [0, 0, 0]
        else:
            assert s == _capi.PPF_ERR_HIP and o.cleared(3, top=rparams(**kw).top), (kw, _capi.last_error())
    for n in (0, 256):
        ptr, n_models = handle
        o = Outputs(max(n, 1), top=2, n_models=n_models)
        arr = (C.c_void_p * max(n, 1))()
        s = lib().ppf_recognize_frame(ptr, arr, n, C.byref(defaults()), o.n_used, o.counts if HAVE_GPU else None, o.ranked, o.n_ranked, C.byref(o.st))
        assert s == (_capi.PPF_OK if HAVE_GPU else _capi.PPF_ERR_HIP), (n, _capi.last_error())
        if n:
            assert list(o.n_ranked) == [0] * n


def test_without_a_device_it_is_loud(handle):
    s, o = frame_call(handle)
    if HAVE_GPU:       # with one the same call succeeds: three NULL clouds, no candidates
        assert s == _capi.PPF_OK and list(o.n_ranked) == [0, 0, 0], _capi.last_error()
        return
    assert s == _capi.PPF_ERR_HIP and o.cleared(3, top=2)
    assert "no HIP device" in _capi.last_error() and "ppf_recognize_frame" in _capi.last_error()
    out = C.c_void_p(7)
    models = (C.c_void_p * 2)(0x10, 0x10)   # never looked into without a device
    assert lib().ppf_recognizer_create(models, 2, C.byref(out)) == _capi.PPF_ERR_HIP and out.value is None
    assert "no HIP device" in _capi.last_error() and "ppf_recognizer_create" in _capi.last_error()


def test_recognizer_handle_errors():
    out = C.c_void_p(7)
    models = (C.c_void_p * 65)(*([0x10] * 65))
    create = lib().ppf_recognizer_create
    assert create(None, 1, C.byref(out)) == _capi.PPF_ERR_INVALID and out.value is None
    for n in (0, -1, 65):
        out = C.c_void_p(7)
        assert create(models, n, C.byref(out)) == _capi.PPF_ERR_INVALID and out.value is None and "n_models" in _capi.last_error()
    assert create(models, 1, None) == _capi.PPF_ERR_INVALID
    holes = (C.c_void_p * 2)(None, None)
    out = C.c_void_p(7)
    assert create(holes, 2, C.byref(out)) == _capi.PPF_ERR_INVALID and out.value is None and "model 0 is NULL" in _capi.last_error()
    assert lib().ppf_recognizer_release(None) == _capi.PPF_OK
    assert lib().ppf_recognizer_retain(None) == _capi.PPF_ERR_INVALID
    info, n = RecognizerInfo(), C.c_int(5)
    assert lib().ppf_recognizer_model_info(None, 0, C.byref(info)) == _capi.PPF_ERR_INVALID
    assert lib().ppf_recognizer_keys(None, 0, None, 0, C.byref(n)) == _capi.PPF_ERR_INVALID


def test_python_wrapper_checks_its_arguments():
    from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, Recognizer
    from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
    with pytest.raises(_capi.PPFError) as e:
        Recognizer([])
    assert e.value.status == _capi.PPF_ERR_INVALID and "n_models" in str(e.value)
    with pytest.raises(_capi.PPFError) as e:
        Recognizer([PPF3DDetector(0.05, 0.05)])   # not trained
    assert e.value.status == _capi.PPF_ERR_NOT_TRAINED
    with pytest.raises(_capi.PPFError) as e:
        CloudProcessor().RecognizeFrame()
    assert e.value.status == _capi.PPF_ERR_NOT_TRAINED


def build_demo(tmp_path, compiler="g++"):
    exe = str(tmp_path / f"recognize_demo_{compiler}")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "recognize_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_demo_compiles_as_cxx11(tmp_path, compiler):
    build_demo(tmp_path, compiler)


def test_demo_fails_loudly_without_gpu(tmp_path):
    exe = build_demo(tmp_path)
    if HAVE_GPU:
        return
    rows = np.ones((8, 6), np.float32)
    (tmp_path / "c.f32").write_bytes(rows.tobytes())
    r = subprocess.run([exe, str(tmp_path / "c.f32"), "8", str(tmp_path / "c.f32"), "8"], capture_output=True, text=True)
    assert r.returncode == 10 + _capi.PPF_ERR_HIP, (r.returncode, r.stderr)
    assert "no HIP device" in r.stderr
