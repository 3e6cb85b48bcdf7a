"""ppf_verify_frame_rendered's and ppf_render_frame's C-ABI surface without a GPU: the two structs as a C compiler lays them
out equal their ctypes mirrors, the defaults, every argument error comes before any device work (zeroed score rows and
best == -1; images left all 0 and all -1), and a valid call fails loudly (PPF_ERR_HIP) when there is no device.  Also the
shape figures of DESIGN.md §15 from the numpy oracle: what the default splat radius and tolerance call hidden."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import render_oracle as R
from test_verify_capi import INTR, _dets
from yolo_ppf_pose_estimation_amd import _capi, synth
from yolo_ppf_pose_estimation_amd._capi import Pose, PoseScore, RenderParams, RenderStats, VerifyParams, VerifyStats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_render_struct_layouts_match_the_header(tmp_path):
    structs = [("ppf_render_params", RenderParams), ("ppf_render_stats", RenderStats)]
    expr, got = [], []
    for cname, cls in structs:
        expr.append(f"sizeof({cname})")
        got.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            expr.append(f"offsetof({cname}, {f})")
            got.append(getattr(cls, f).offset)
    expr += ["PPF_RENDER_MAX_SPLAT", "PPF_ABI_VERSION"]
    got += [_capi.PPF_RENDER_MAX_SPLAT, 4]
    src = tmp_path / "rsz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppf_hip.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "rsz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert R.MAX_SPLAT == _capi.PPF_RENDER_MAX_SPLAT


def rdefaults():
    p = RenderParams()
    p.splat_radius, p.visible_tol, p.flags = 7.0, 7.0, 7
    for i in range(4):
        p.reserved[i] = 7
    lib().ppf_default_render_params(C.byref(p))
    return p


def vdefaults():
    p = VerifyParams()
    lib().ppf_default_verify_params(C.byref(p))
    return p


def test_render_defaults():
    p = rdefaults()
    assert (p.splat_radius, p.visible_tol, p.flags) == (C.c_float(0.003).value, C.c_float(0.005).value, 0)
    assert list(p.reserved) == [0, 0, 0, 0]
    lib().ppf_default_render_params(None)   # no crash


# ---- ppf_verify_frame_rendered -------------------------------------------------------------------------------------------
def _vcall(dets, n_dets, n_poses=None, top=4, depth=None, rows=480, cols=640, intr=INTR, p=None, rp=None, poses=True, counts=True,
           scores=True, best=True, params=True, rparams=True):
    np_ = (C.c_int * 300)(*([2] * 300 if n_poses is None else n_poses))
    ps = (Pose * (300 * 16))() if poses else None
    sc = (PoseScore * (300 * 16))()
    for i in range(len(sc)):
        sc[i].n_rows, sc[i].score = 77, 7.0   # garbage the call must clear
    bs = (C.c_int * 300)(*([55] * 300))
    it = (C.c_double * 4)(*intr) if intr is not None else None
    prm = vdefaults() if p is None else p
    rprm = rdefaults() if rp is None else rp
    st = VerifyStats()
    st.n_launches = 99
    s = lib().ppf_verify_frame_rendered(dets, n_dets, ps, np_ if counts else None, top, depth, rows, cols, it,
                                        C.byref(prm) if params else None, C.byref(rprm) if rparams else None, sc if scores else None,
                                        bs if best else None, C.byref(st))
    return s, sc, bs, st


def _cleared(sc, bs, n_dets, top=4):
    return all(bytes(sc[i]) == bytes(PoseScore()) for i in range(n_dets * top)) and list(bs[:n_dets]) == [-1] * n_dets and \
        sc[n_dets * top].n_rows == 77 and bs[n_dets] == 55


def _vinvalid(r, n_dets=3, top=4, needle=None):
    s, sc, bs, st = r
    assert s == _capi.PPF_ERR_INVALID, (s, _capi.last_error())
    assert "ppf_verify_frame_rendered" in _capi.last_error()
    if needle:
        assert needle in _capi.last_error(), _capi.last_error()
    assert st.n_launches == 0 and st.n_host_syncs == 0 and st.n_jobs == 0
    if 0 < n_dets <= 256 and 1 <= top <= 16:
        assert _cleared(sc, bs, n_dets, top)


def test_verify_rendered_range_and_null_errors():
    dets = _dets(3)
    _vinvalid(_vcall(dets, 257), n_dets=257, needle="n_dets")
    _vinvalid(_vcall(dets, -1), n_dets=-1, needle="n_dets")
    for top in (0, 17):
        _vinvalid(_vcall(dets, 3, top=top), top=top, needle="top")
    _vinvalid(_vcall(dets, 3, n_poses=[2, 5, 1]), needle="n_poses[1]")
    _vinvalid(_vcall(dets, 3, params=False), needle="params")
    _vinvalid(_vcall(dets, 3, rparams=False), needle="rparams")
    _vinvalid(_vcall(dets, 3, poses=False))
    _vinvalid(_vcall(dets, 3, counts=False))
    _vinvalid(_vcall(None, 3))
    _vinvalid(_vcall(_dets(3, model_cloud=False), 3), needle="detection 0")
    _vinvalid(_vcall(_dets(3, scene=False), 3), needle="detection 0")


def test_verify_rendered_parameter_errors():
    dets = _dets(3)
    for field, values in (("inlier_dist", (0.0, NAN)), ("normal_cos", (1.5,)), ("depth_tol", (0.0, INF)), ("model_step", (0,)),
                          ("flags", (4, 8, -1))):
        for v in values:
            p = vdefaults()
            setattr(p, field, v)
            _vinvalid(_vcall(dets, 3, p=p))
    for flags in (_capi.PPF_VERIFY_ALL_ROWS, _capi.PPF_VERIFY_ALL_ROWS | _capi.PPF_VERIFY_NORMALS):
        p = vdefaults()
        p.flags = flags
        _vinvalid(_vcall(dets, 3, p=p), needle="PPF_VERIFY_ALL_ROWS")
    for field, values in (("splat_radius", (0.0, -0.001, NAN, INF)), ("visible_tol", (0.0, -1.0, NAN, INF)), ("flags", (1, -1, 4))):
        for v in values:
            rp = rdefaults()
            setattr(rp, field, v)
            _vinvalid(_vcall(dets, 3, rp=rp), needle=field)


def test_verify_rendered_needs_the_image():
    """without a depth image the image size and intr are still required; fx and fy must be > 0"""
    dets = _dets(3)
    for rows, cols in ((0, 640), (480, 0), (-1, 4), (70000, 70000)):
        _vinvalid(_vcall(dets, 3, rows=rows, cols=cols))
    _vinvalid(_vcall(dets, 3, intr=None), needle="intr")
    for bad in ((0.0, 1.0, 2.0, 2.0), (1.0, -1.0, 2.0, 2.0), (-5.0, 1.0, 2.0, 2.0), (NAN, 1.0, 2.0, 2.0), (1.0, INF, 2.0, 2.0),
                (1.0, 1.0, NAN, 2.0), (1.0, 1.0, 2.0, -INF)):
        _vinvalid(_vcall(dets, 3, intr=bad))
    img = (C.c_float * 16)()
    _vinvalid(_vcall(dets, 3, depth=img, rows=4, cols=4, intr=(-1000.0, 1000.0, 2.0, 2.0)), needle="fx and fy")
    _vinvalid(_vcall(dets, 3, depth=img, rows=0, cols=4))


def test_verify_rendered_without_a_device_is_loud():
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    img = (C.c_float * 16)()
    for n, kw in ((0, {}), (3, {}), (3, dict(depth=img, rows=4, cols=4)), (3, dict(p=_flags(_capi.PPF_VERIFY_NORMALS)))):
        s, sc, bs, st = _vcall(_dets(n), n, **kw)
        assert s == _capi.PPF_ERR_HIP
        assert "no HIP device" in _capi.last_error() and "ppf_verify_frame_rendered" in _capi.last_error()
        assert st.n_launches == 0 and st.n_host_syncs == 0
        if n:
            assert _cleared(sc, bs, n)


def _flags(f):
    p = vdefaults()
    p.flags = f
    return p


# ---- ppf_render_frame -----------------------------------------------------------------------------------------------------
def _rcall(dets, n_dets, which=None, top=4, rows=6, cols=5, intr=INTR, rp=None, poses=True, whiches=True, rparams=True, images=True):
    ws = (C.c_int * 300)(*([1] * 300 if which is None else which))
    ps = (Pose * (300 * 16))() if poses else None
    it = (C.c_double * 4)(*intr) if intr is not None else None
    rprm = rdefaults() if rp is None else rp
    n = max(rows * cols, 1) if 0 < rows < 100 and 0 < cols < 100 else 1
    depth = np.full(n + 1, 9.0, dtype=np.float32)
    label = np.full(n + 1, 9, dtype=np.int32)
    st = RenderStats()
    st.n_launches = 99
    s = lib().ppf_render_frame(dets, n_dets, ps, ws if whiches else None, top, rows, cols, it, C.byref(rprm) if rparams else None,
                               depth.ctypes.data if images else None, label.ctypes.data if images else None, C.byref(st))
    return s, depth, label, st


def _rinvalid(r, needle=None, sized=True):
    s, depth, label, st = r
    assert s == _capi.PPF_ERR_INVALID, (s, _capi.last_error())
    assert "ppf_render_frame" in _capi.last_error()
    if needle:
        assert needle in _capi.last_error(), _capi.last_error()
    assert st.n_launches == 0 and st.n_host_syncs == 0 and st.n_jobs == 0
    if sized:   # the images are cleared, nothing beyond them is touched
        assert (depth[:-1] == 0).all() and (label[:-1] == -1).all() and depth[-1] == 9.0 and label[-1] == 9


def test_render_frame_argument_errors():
    dets = _dets(3)
    _rinvalid(_rcall(dets, 257), needle="n_dets")
    _rinvalid(_rcall(dets, -1), needle="n_dets")
    for top in (0, 17):
        _rinvalid(_rcall(dets, 3, top=top), needle="top")
    _rinvalid(_rcall(dets, 3, which=[0, 4, -1]), needle="which[1]")
    _rinvalid(_rcall(dets, 3, which=[0, -2, 1]), needle="which[1]")
    _rinvalid(_rcall(dets, 3, which=[0, 1, 16], top=16), needle="which[2]")
    _rinvalid(_rcall(_dets(3, model_cloud=False), 3, which=[-1, 2, -1]), needle="detection 1")
    _rinvalid(_rcall(dets, 3, poses=False))
    _rinvalid(_rcall(dets, 3, whiches=False))
    _rinvalid(_rcall(None, 3))
    _rinvalid(_rcall(dets, 3, rparams=False), needle="rparams")
    for field, values in (("splat_radius", (0.0, -0.001, NAN, INF)), ("visible_tol", (0.0, NAN)), ("flags", (1, -1))):
        for v in values:
            rp = rdefaults()
            setattr(rp, field, v)
            _rinvalid(_rcall(dets, 3, rp=rp), needle=field)
    _rinvalid(_rcall(dets, 3, intr=None), needle="intr")
    for bad in ((0.0, 1.0, 2.0, 2.0), (1.0, -1.0, 2.0, 2.0), (NAN, 1.0, 2.0, 2.0), (1.0, 1.0, INF, 2.0)):
        _rinvalid(_rcall(dets, 3, intr=bad))
    for rows, cols in ((0, 5), (6, 0), (-1, 5), (70000, 70000)):
        _rinvalid(_rcall(dets, 3, rows=rows, cols=cols), sized=False)
    s, *_ = _rcall(dets, 3, intr=None, images=False)   # NULL images are allowed, the error still comes
    assert s == _capi.PPF_ERR_INVALID


def test_render_frame_without_a_device_is_loud():
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    for n, which in ((0, None), (3, [0, -1, 3]), (3, [-1, -1, -1])):
        s, depth, label, st = _rcall(_dets(n), n, which=which)
        assert s == _capi.PPF_ERR_HIP, _capi.last_error()
        assert "no HIP device" in _capi.last_error() and "ppf_render_frame" in _capi.last_error()
        assert st.n_launches == 0 and st.n_host_syncs == 0
        assert (depth[:-1] == 0).all() and (label[:-1] == -1).all()


# ---- the shape figures that fix the defaults (numpy oracle, a numpy transform) ---------------------------------------------
INTR_SYNTH = (460.0, 460.0, 319.5, 179.5)


def _tilt(deg, c=(0.0, 0.0, 0.6)):
    t = math.radians(deg)
    Rx = np.array([[1, 0, 0], [0, math.cos(t), -math.sin(t)], [0, math.sin(t), math.cos(t)]])
    T = np.eye(4)
    T[:3, :3] = Rx
    T[:3, 3] = np.asarray(c) - Rx @ np.asarray(c)
    return T


@pytest.mark.parametrize("kind,deg,lo,hi", [("box", 0, 0.0, 0.01), ("box", 50, 0.0, 0.01), ("cylinder", 50, 0.0, 0.05),
                                            ("cylinder", 70, 0.0, 0.05), ("torus", 50, 0.0, 0.05), ("torus", 85, 0.30, 1.0)])
def test_default_splat_hides_what_is_hidden(kind, deg, lo, hi):
    p = rdefaults()
    o = R.move_np(synth.make_solid(kind, 20000, seed=7), _tilt(deg))
    share = R.hidden_share(o, 360, 640, INTR_SYNTH, p.splat_radius, p.visible_tol)
    assert lo <= share <= hi, (kind, deg, share)
