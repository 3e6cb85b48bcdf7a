"""ppf_depth_edges' C-ABI surface without a GPU: the symbols are exported and bound, both records as a C++ compiler lays them
out equal their ctypes mirrors, the defaults, every argument error comes before any device work in the order the header states
(and leaves *out_cloud NULL and the stats zero), the ends of every range are accepted, the call fails loudly (PPF_ERR_HIP) when
there is no device, and the demo is C++11 for g++ and clang++."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import DepthEdgeParams, DepthEdgeStats, DepthParams, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
PARAM_FIELDS = ["depth_abs", "depth_quad", "max_gap", "curvature_threshold", "select", "flags", "reserved"]
STATS_FIELDS = ["n_kept", "n_occluding", "n_occluded", "n_boundary", "n_curvature", "n_edge", "n_selected", "n_no_normal", "n_rows",
                "n_launches", "n_host_syncs", "ms_wall", "reserved"]
ENTRIES = ["ppf_default_depth_edge_params", "ppf_depth_edges", "ppf_depth_edges_device"]
INTR = (500.0, 500.0, 3.0, 2.0)
DIRTY = 0x5A5A5A5A


def test_symbols_are_exported_and_bound():
    raw = C.CDLL(_capi.LIB_PATH)   # a handle of its own: nothing is bound on it yet
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _capi._SIGNATURES, name
        res, args = _capi._SIGNATURES[name]
        assert list(getattr(lib(), name).argtypes) == list(args) and getattr(lib(), name).restype == res, name


def test_records_and_defaults_match_the_header(tmp_path):
    src = tmp_path / "desz.cpp"
    expr = ["sizeof(ppf_depth_edge_params)"] + [f"offsetof(ppf_depth_edge_params, {f})" for f in PARAM_FIELDS] + \
           ["sizeof(ppf_depth_edge_stats)"] + [f"offsetof(ppf_depth_edge_stats, {f})" for f in STATS_FIELDS] + \
           ["PPF_EDGE_OCCLUDING", "PPF_EDGE_OCCLUDED", "PPF_EDGE_BOUNDARY", "PPF_EDGE_CURVATURE", "PPF_DEPTH_EDGE_MAX_GAP", "PPF_ABI_VERSION"]
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ppf_hip.h"\nint main(){\n' +
                   "".join(f'std::printf("%zu\\n", (size_t)({e}));\n' for e in expr) +
                   "ppf_depth_edge_params p; ppf_default_depth_edge_params(&p);\n"
                   'std::printf("%a %a %d %a %d %d\\n", p.depth_abs, p.depth_quad, p.max_gap, p.curvature_threshold, p.select, p.flags);\n'
                   "return 0;}\n")
    exe = tmp_path / "desz"
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", CSRC, "-lppf_hip",
                    f"-Wl,-rpath,{CSRC}", "-o", str(exe)], check=True)
    words = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    want = [int(v) for v in words[:-6]]
    got = [C.sizeof(DepthEdgeParams)] + [getattr(DepthEdgeParams, f).offset for f in PARAM_FIELDS] + \
          [C.sizeof(DepthEdgeStats)] + [getattr(DepthEdgeStats, f).offset for f in STATS_FIELDS] + \
          [_capi.PPF_EDGE_OCCLUDING, _capi.PPF_EDGE_OCCLUDED, _capi.PPF_EDGE_BOUNDARY, _capi.PPF_EDGE_CURVATURE, _capi.PPF_DEPTH_EDGE_MAX_GAP,
           _capi.PPF_ABI_VERSION]
    assert got == want
    assert want[-6:] == [1, 2, 4, 8, 8, 4]                   # the interface only grows: the ABI version stays
    assert [f for f, _ in DepthEdgeParams._fields_] == PARAM_FIELDS and [f for f, _ in DepthEdgeStats._fields_] == STATS_FIELDS
    p = defaults()
    mine = [float(p.depth_abs).hex(), float(p.depth_quad).hex(), p.max_gap, float(p.curvature_threshold).hex(), p.select, p.flags]
    theirs = [float.fromhex(words[-6]).hex(), float.fromhex(words[-5]).hex(), int(words[-4]), float.fromhex(words[-3]).hex(), int(words[-2]),
              int(words[-1])]
    assert mine == theirs


def depth_defaults():
    p = DepthParams()
    lib().ppf_default_depth_params(C.byref(p))
    return p


def defaults():
    p = DepthEdgeParams()
    p.depth_abs, p.depth_quad, p.max_gap, p.curvature_threshold, p.select, p.flags = 7.0, 7.0, 7, 7.0, 7, 7
    for i in range(4):
        p.reserved[i] = 7
    lib().ppf_default_depth_edge_params(C.byref(p))
    return p


def test_defaults():
    p = defaults()
    f = lambda v: float(np.float32(v))  # noqa: E731
    assert (p.depth_abs, p.depth_quad, p.max_gap, p.curvature_threshold, p.select, p.flags) == (f(0.02), 0.0, 2, f(0.03), 1 | 4 | 8, 0)
    assert list(p.reserved) == [0, 0, 0, 0]
    lib().ppf_default_depth_edge_params(None)   # no crash


def eparams(**kw):
    p = defaults()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def dparams(**kw):
    p = depth_defaults()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def dirty_stats():
    st = DepthEdgeStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    return st


def stats_are_zero(st):
    return bytes(st) == bytes(C.sizeof(st))


def host_call(img, rows=4, cols=6, pitch=0, intr=INTR, dp=None, ep=None, edges=True, cloud=False, stats=True):
    """-> (status, stats, the edges buffer, *out_cloud as an int or None)"""
    dprm = depth_defaults() if dp is None else dp
    eprm = defaults() if ep is None else ep
    res = np.full((max(rows, 1), max(cols, 1)), np.uint8(7)) if rows * cols < 1 << 20 else np.zeros(1, np.uint8)
    st = dirty_stats()
    found = C.c_void_p(DIRTY)
    it = (C.c_double * 4)(*intr) if intr is not None else None
    s = lib().ppf_depth_edges(C.c_void_p(img.ctypes.data) if img is not None else None, rows, cols, pitch, it,
                              C.byref(dprm) if dprm is not False else None, None, C.byref(eprm) if eprm is not False else None,
                              C.c_void_p(res.ctypes.data) if edges else None, C.byref(found) if cloud else None, C.byref(st) if stats else None)
    return s, st, res, found.value


def device_call(rows=4, cols=6, pitch=0, intr=INTR, dp=None, ep=None, ptr=0x10, edges=0x100000, cloud=False):
    """the device entry with arguments that are rejected before a pointer is looked at (neither is ever read)"""
    dprm = depth_defaults() if dp is None else dp
    eprm = defaults() if ep is None else ep
    st = dirty_stats()
    found = C.c_void_p(DIRTY)
    it = (C.c_double * 4)(*intr) if intr is not None else None
    s = lib().ppf_depth_edges_device(C.c_void_p(ptr) if ptr else None, rows, cols, pitch, it, C.byref(dprm) if dprm is not False else None, None,
                                     C.byref(eprm) if eprm is not False else None, C.c_void_p(edges) if edges else None, None,
                                     C.byref(found) if cloud else None, C.byref(st))
    return s, st, found.value


def edge_cases():
    """the errors the entry adds to ppf_cloud_from_depth's"""
    return [
        ("NULL edge params", dict(ep=False)),
        ("depth_abs < 0", dict(ep=eparams(depth_abs=-0.01))),
        ("depth_abs nan", dict(ep=eparams(depth_abs=math.nan))),
        ("depth_abs inf", dict(ep=eparams(depth_abs=math.inf))),
        ("depth_quad < 0", dict(ep=eparams(depth_quad=-1.0))),
        ("depth_quad nan", dict(ep=eparams(depth_quad=math.nan))),
        ("depth_quad inf", dict(ep=eparams(depth_quad=math.inf))),
        ("max_gap -1", dict(ep=eparams(max_gap=-1))),
        ("max_gap 9", dict(ep=eparams(max_gap=9))),
        ("curvature_threshold < 0", dict(ep=eparams(curvature_threshold=-0.5))),
        ("curvature_threshold nan", dict(ep=eparams(curvature_threshold=math.nan))),
        ("select 0", dict(ep=eparams(select=0))),
        ("select 16", dict(ep=eparams(select=16))),
        ("select 31", dict(ep=eparams(select=31))),
        ("select -1", dict(ep=eparams(select=-1))),
        ("flags 1", dict(ep=eparams(flags=1))),
        ("unknown depth flag", dict(dp=dparams(flags=2))),
        ("unknown depth flags", dict(dp=dparams(flags=_capi.PPF_DEPTH_FP64 | 4))),
    ]


def depth_cases():
    """ppf_cloud_from_depth's own errors, through the new entry"""
    f32 = np.zeros((4, 6), np.float32)
    u16 = np.zeros((4, 6), np.uint16)
    odd = np.zeros(64, np.uint8)[1:]
    return [
        ("NULL depth", dict(img=None)),
        ("NULL depth params", dict(img=f32, dp=False)),
        ("rows 0", dict(img=f32, rows=0)),
        ("cols -1", dict(img=f32, cols=-1)),
        ("rows * cols > INT32_MAX", dict(img=f32, rows=65536, cols=32768)),
        ("pitch below the row", dict(img=f32, pitch=20)),
        ("pitch not a multiple", dict(img=f32, pitch=26)),
        ("u16 pitch odd", dict(img=u16, pitch=13, dp=dparams(format=_capi.PPF_DEPTH_U16))),
        ("misaligned image", dict(img=odd, rows=2, cols=3, dp=dparams(format=_capi.PPF_DEPTH_U16))),
        ("format 2", dict(img=f32, dp=dparams(format=2))),
        ("u16 scale 0", dict(img=u16, dp=dparams(format=_capi.PPF_DEPTH_U16, depth_scale=0.0))),
        ("u16 scale nan", dict(img=u16, dp=dparams(format=_capi.PPF_DEPTH_U16, depth_scale=math.nan))),
        ("z_min inf", dict(img=f32, dp=dparams(z_min=math.inf))),
        ("z_max nan", dict(img=f32, dp=dparams(z_max=math.nan))),
        ("z_max < 0", dict(img=f32, dp=dparams(z_max=-1.0))),
    ]


@pytest.mark.parametrize("cloud", [False, True])
@pytest.mark.parametrize("name,kw", edge_cases(), ids=[c[0] for c in edge_cases()])
def test_edge_argument_errors_precede_any_device_work(name, kw, cloud):
    s, st, res, found = host_call(np.ones((4, 6), np.float32), cloud=cloud, **kw)
    assert s == _capi.PPF_ERR_INVALID, (name, _capi.last_error())
    assert stats_are_zero(st) and (res == 7).all() and found == (None if cloud else DIRTY), name
    assert "ppf_depth_edges:" in _capi.last_error()
    s, st, found = device_call(cloud=cloud, **kw)
    assert s == _capi.PPF_ERR_INVALID and stats_are_zero(st) and found == (None if cloud else DIRTY), (name, _capi.last_error())
    assert "ppf_depth_edges_device:" in _capi.last_error()


@pytest.mark.parametrize("name,kw", depth_cases(), ids=[c[0] for c in depth_cases()])
def test_depth_argument_errors_are_kept(name, kw):
    s, st, _, found = host_call(cloud=True, **kw)
    assert s == _capi.PPF_ERR_INVALID, (name, _capi.last_error())
    assert stats_are_zero(st) and found is None, name
    assert "ppf_depth_edges:" in _capi.last_error()
    dkw = {k: v for k, v in kw.items() if k != "img"}
    if kw.get("img", 1) is None:
        dkw["ptr"] = 0
    elif name == "misaligned image":
        dkw["ptr"] = 0x11
    s, st, _ = device_call(**dkw)
    assert s == _capi.PPF_ERR_INVALID and stats_are_zero(st), (name, _capi.last_error())
    assert "ppf_depth_edges_device:" in _capi.last_error()


def test_outputs_and_intr():
    img = np.ones((4, 6), np.float32)
    s, st, res, _ = host_call(img, edges=False)                        # nothing to write to
    assert s == _capi.PPF_ERR_INVALID and stats_are_zero(st) and "both NULL" in _capi.last_error()
    s, st, _ = device_call(edges=0)
    assert s == _capi.PPF_ERR_INVALID and stats_are_zero(st) and "both NULL" in _capi.last_error()
    s, st, _, found = host_call(img, intr=None, cloud=True)            # a cloud without normals needs the camera
    assert s == _capi.PPF_ERR_INVALID and stats_are_zero(st) and found is None and "intr" in _capi.last_error()
    for bad in ((0.0, 500.0, 3.0, 2.0), (500.0, math.nan, 3.0, 2.0), (500.0, 500.0, math.inf, 2.0)):
        s, st, _, found = host_call(img, intr=bad, cloud=True)
        assert s == _capi.PPF_ERR_INVALID and stats_are_zero(st) and found is None, bad
        s, _, _, _ = host_call(img, intr=bad)                          # the mask alone never reads it
        assert s != _capi.PPF_ERR_INVALID, (bad, _capi.last_error())
    s, _, _, _ = host_call(img, intr=None)
    assert s != _capi.PPF_ERR_INVALID, _capi.last_error()
    s, _, _, _ = host_call(img, ep=eparams(max_gap=9), stats=False)    # no crash without stats
    assert s == _capi.PPF_ERR_INVALID


def test_the_order_of_the_checks():
    """outputs, ep NULL and a missing intr come before the image; the image (with dp's flags) and intr's values before the z
    range; the z range before ep's fields"""
    img = np.ones((4, 6), np.float32)
    bad_ep = eparams(max_gap=9)
    for kw, word in ((dict(edges=False, ep=False, img=None), "both NULL"), (dict(ep=False, img=None), "edge params"),
                     (dict(intr=None, cloud=True, img=None), "intr"), (dict(img=None, ep=bad_ep), "must not be NULL"),
                     (dict(rows=0, dp=dparams(flags=2), ep=bad_ep), "0 x 6"), (dict(dp=dparams(flags=2), pitch=20, ep=bad_ep), "flags"),
                     (dict(pitch=20, intr=(0.0, 1.0, 0.0, 0.0), cloud=True, ep=bad_ep), "pitch"),
                     (dict(intr=(0.0, 1.0, 0.0, 0.0), cloud=True, dp=dparams(z_max=-1.0), ep=bad_ep), "fx"),
                     (dict(dp=dparams(z_max=-1.0), ep=bad_ep), "z_min"), (dict(ep=eparams(depth_abs=-1.0, max_gap=9)), "depth_abs"),
                     (dict(ep=eparams(max_gap=9, curvature_threshold=-1.0)), "max_gap"),
                     (dict(ep=eparams(curvature_threshold=-1.0, select=0)), "curvature_threshold"), (dict(ep=eparams(select=0, flags=1)), "select")):
        kw = dict(kw)
        s, st, _, _ = host_call(kw.pop("img", img), **kw)
        assert s == _capi.PPF_ERR_INVALID and word in _capi.last_error(), (word, _capi.last_error())


def test_range_edges_and_fp64_reach_the_device_check():
    """the ends of every range pass the argument checks: the status is not PPF_ERR_INVALID"""
    img = np.ones((4, 6), np.float32)
    img[1, 2] = 0
    for kw in (dict(max_gap=0), dict(max_gap=8), dict(depth_abs=0.0, depth_quad=0.0), dict(curvature_threshold=0.0),
               dict(curvature_threshold=math.inf), dict(select=1), dict(select=15)):
        s, st, res, _ = host_call(img, ep=eparams(**kw))
        if lib().ppf_device_count() > 0:
            assert s == _capi.PPF_OK and st.n_kept == 23 and (st.n_launches, st.n_host_syncs) == (1, 1), (kw, _capi.last_error())
        else:
            assert s == _capi.PPF_ERR_HIP and stats_are_zero(st) and (res == 7).all(), (kw, _capi.last_error())
    s, _, _, _ = host_call(img, dp=dparams(flags=_capi.PPF_DEPTH_FP64), cloud=True)
    assert s != _capi.PPF_ERR_INVALID, _capi.last_error()


def test_without_a_device_it_is_loud():
    img = np.ones((4, 6), np.float32)
    s, st, res, found = host_call(img, cloud=True)
    if lib().ppf_device_count() > 0:       # with one the same call succeeds: a constant image has no edge
        assert s == _capi.PPF_OK and not res.any() and st.n_rows == 0, _capi.last_error()
        assert lib().ppf_cloud_release(C.c_void_p(found)) == _capi.PPF_OK
        return
    assert s == _capi.PPF_ERR_HIP and stats_are_zero(st) and (res == 7).all() and found is None
    assert "no HIP device" in _capi.last_error() and "ppf_depth_edges" in _capi.last_error()
    s, st, found = device_call(cloud=True)
    assert s == _capi.PPF_ERR_HIP and stats_are_zero(st) and found is None
    assert "ppf_depth_edges_device" in _capi.last_error()


def build_demo(tmp_path, compiler="g++"):
    exe = str(tmp_path / f"depth_edges_demo_{compiler}")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "depth_edges_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_demo_compiles_as_cxx11(tmp_path, compiler):
    build_demo(tmp_path, compiler)


def test_demo_fails_loudly_without_gpu(tmp_path):
    exe = build_demo(tmp_path)
    if lib().ppf_device_count() > 0:
        return
    (tmp_path / "d.f32").write_bytes(np.ones((4, 6), np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "d.f32"), "4", "6", "500", "500", "3", "2"], capture_output=True, text=True)
    assert r.returncode == 10 + _capi.PPF_ERR_HIP, (r.returncode, r.stderr)
    assert "ppf_depth_edges" in r.stderr


def test_python_wrapper_rejects_unknown_keys_and_other_dtypes():
    from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, depth_edges
    img = np.ones((4, 6), np.float32)
    for call in (lambda: depth_edges(img, params=dict(max_gab=3)), lambda: depth_edges(np.zeros((4, 6), np.float64)),
                 lambda: depth_edges(np.zeros((2, 4, 6), np.float32)), lambda: depth_edges(img, out=np.zeros((4, 5), np.uint8)),
                 lambda: depth_edges(img, out=np.zeros((4, 6), np.int32)), lambda: depth_edges(img, normals=np.zeros((3, 6), np.float32)),
                 lambda: DeviceCloud.from_depth(img, INTR, edges=dict(max_gab=3)) if lib().ppf_device_count() > 0 else depth_edges(img, params=dict(x=1)),
                 lambda: CloudProcessor(None, None).EdgeExtractionDepth()):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID
    with pytest.raises(_capi.PPFError) as e:
        depth_edges(img, params=dict(max_gap=9))
    assert e.value.status == _capi.PPF_ERR_INVALID and "max_gap" in str(e.value)
    with pytest.raises(_capi.PPFError) as e:
        depth_edges(img, cloud=True)
    assert e.value.status == _capi.PPF_ERR_INVALID and "intr" in str(e.value)
