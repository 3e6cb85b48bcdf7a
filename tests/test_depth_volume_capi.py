"""ppf_depth_volume's C-ABI surface without a GPU: the symbols are exported and bound, the records as a C++ and a C compiler lay
them out equal their ctypes mirrors, the defaults, every argument error of every entry is PPF_ERR_INVALID before any device
work with the outputs as the header states them (untouched images, *out NULL, zero stats) and in the order the header states,
the ends of every range get past the checks, and without a device a valid call is PPF_ERR_HIP.

Without a device nothing can be created, and the entries must still refuse their arguments first.  There they are handed a
shell (ppf_debug_depth_volume_shell): a handle with the parameters and no device memory.  With a device the volume is a real
one."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import (DepthParams, DepthVolumeDesc, DepthVolumeExtractParams, DepthVolumeExtractStats,
                                                DepthVolumeIntegrateStats, DepthVolumeParams, DepthVolumeRaycastParams,
                                                DepthVolumeRaycastStats, lib)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_GPU = lib().ppf_device_count() > 0
ENTRIES = ["ppf_default_depth_volume_params", "ppf_default_depth_volume_raycast_params", "ppf_default_depth_volume_extract_params",
           "ppf_depth_volume_create", "ppf_debug_depth_volume_shell", "ppf_depth_volume_release", "ppf_depth_volume_reset", "ppf_depth_volume_info", "ppf_depth_volume_read",
           "ppf_depth_volume_integrate", "ppf_depth_volume_integrate_device", "ppf_depth_volume_raycast", "ppf_depth_volume_raycast_device",
           "ppf_depth_volume_extract"]
RECORDS = [
    ("ppf_depth_volume_params", DepthVolumeParams, ["dims", "voxel", "origin", "trunc", "max_weight", "flags", "reserved"]),
    ("ppf_depth_volume_desc", DepthVolumeDesc, ["dims", "voxel", "origin", "trunc", "max_weight", "integrations", "device_bytes", "reserved"]),
    ("ppf_depth_volume_integrate_stats", DepthVolumeIntegrateStats, ["n_updated", "n_launches", "n_host_syncs", "ms_wall", "reserved"]),
    ("ppf_depth_volume_raycast_params", DepthVolumeRaycastParams, ["z_near", "z_far", "ray_step", "min_weight", "flags", "reserved"]),
    ("ppf_depth_volume_raycast_stats", DepthVolumeRaycastStats, ["n_hits", "n_interpolated", "n_launches", "n_host_syncs", "ms_wall", "reserved"]),
    ("ppf_depth_volume_extract_params", DepthVolumeExtractParams, ["min_weight", "flags", "reserved"]),
    ("ppf_depth_volume_extract_stats", DepthVolumeExtractStats, ["n_crossings", "n_rows", "n_launches", "n_host_syncs", "ms_wall", "reserved"]),
]
ROWS, COLS = 12, 20
INTR = (20.0, 20.0, 9.5, 5.5)
EYE = np.eye(4).reshape(-1)
IMG = np.full((ROWS, COLS), 0.7, np.float32)
IMG16 = np.full((ROWS, COLS), 700, np.uint16)


def test_symbols_are_exported_and_bound():
    raw = C.CDLL(_capi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        res, args = _capi._SIGNATURES[name]
        assert list(getattr(lib(), name).argtypes) == list(args) and getattr(lib(), name).restype == res, name


def test_records_match_the_header(tmp_path):
    consts = ["PPF_VOLUME_MAX_DIM", "PPF_VOLUME_MAX_WEIGHT", "PPF_VOLUME_MAX_STEPS", "PPF_VOLUME_MAX_TILES", "PPF_ABI_VERSION"]
    expr, got = ["sizeof(ppf_depth_volume_voxel)", "offsetof(ppf_depth_volume_voxel, w)"], [8, 4]
    for cname, cls, fields in RECORDS:
        expr += [f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields]
        got += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
        assert [f for f, _ in cls._fields_] == fields and fields[-1] == "reserved" and C.sizeof(cls._fields_[-1][1]) == 16
    expr += consts
    got += [getattr(_capi, c) for c in consts]
    src = tmp_path / "dvsz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ppf_hip.h"\nint main(){\n' +
                   "".join(f'std::printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "dvsz"
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert want[-5:] == [1024, 65535, 4096, (1 << 24) - 1, 4]   # the interface only grows: the ABI version stays
    csrc = tmp_path / "dvsz.c"
    csrc.write_text('#include <stdio.h>\n#include "ppf_hip.h"\nint main(void){printf("' + "%zu " * len(RECORDS) + '\\n", ' +
                    ", ".join(f"sizeof({c})" for c, _, _ in RECORDS) + ");return 0;}\n")
    cexe = tmp_path / "dvszc"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(cexe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(cexe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(cls) for _, cls, _ in RECORDS]


def vparams(**kw):
    p = DepthVolumeParams()
    C.memset(C.byref(p), 0x09, C.sizeof(p))
    lib().ppf_default_depth_volume_params(C.byref(p))
    for k, v in kw.items():
        if k in ("dims", "origin"):
            getattr(p, k)[:] = v
        else:
            setattr(p, k, v)
    return p


def rparams(**kw):
    p = DepthVolumeRaycastParams()
    C.memset(C.byref(p), 0x09, C.sizeof(p))
    lib().ppf_default_depth_volume_raycast_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def xparams(**kw):
    p = DepthVolumeExtractParams()
    C.memset(C.byref(p), 0x09, C.sizeof(p))
    lib().ppf_default_depth_volume_extract_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def dparams(**kw):
    p = DepthParams()
    lib().ppf_default_depth_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults():
    f = lambda v: float(np.float32(v))
    p = vparams()
    assert list(p.dims) == [256, 256, 256] and p.voxel == f(0.004) and list(p.origin) == [-0.510, -0.510, 0.302]
    assert (p.trunc, p.max_weight, p.flags) == (f(0.016), 64, 0) and list(p.reserved) == [0, 0, 0, 0]
    r = rparams()
    assert (r.z_near, r.z_far, r.ray_step, r.min_weight, r.flags) == (f(0.3), f(1.5), 0.5, 1, 0) and list(r.reserved) == [0, 0, 0, 0]
    x = xparams()
    assert (x.min_weight, x.flags) == (1, 0) and list(x.reserved) == [0, 0, 0, 0]
    for fn in ("ppf_default_depth_volume_params", "ppf_default_depth_volume_raycast_params", "ppf_default_depth_volume_extract_params"):
        getattr(lib(), fn)(None)   # no crash
    import depth_volume_oracle as O
    assert O.VOLUME_DEFAULTS == dict(dims=(256, 256, 256), voxel=0.004, origin=(-0.510, -0.510, 0.302), trunc=0.016, max_weight=64)
    assert O.RAYCAST_DEFAULTS == dict(z_near=0.3, z_far=1.5, ray_step=0.5, min_weight=1) and O.MAX_STEPS == _capi.PPF_VOLUME_MAX_STEPS


# ---- create ---------------------------------------------------------------------------------------------------------------
CREATE_INVALID = [
    ("dims 0", dict(dims=(0, 8, 8)), "dims[0]"),
    ("dims 1025", dict(dims=(8, 8, 1025)), "dims[2]"),
    ("dims < 0", dict(dims=(8, -1, 8)), "dims[1]"),
    ("voxel 0", dict(voxel=0.0), "voxel"),
    ("voxel nan", dict(voxel=math.nan), "voxel"),
    ("voxel inf", dict(voxel=math.inf), "voxel"),
    ("origin nan", dict(origin=(0.0, math.nan, 0.0)), "origin"),
    ("origin inf", dict(origin=(0.0, 0.0, -math.inf)), "origin"),
    ("trunc below voxel", dict(trunc=0.003), "trunc"),
    ("trunc inf", dict(trunc=math.inf), "trunc"),
    ("trunc nan", dict(trunc=math.nan), "trunc"),
    ("max_weight 0", dict(max_weight=0), "max_weight"),
    ("max_weight 65536", dict(max_weight=65536), "max_weight"),
    ("flags 1", dict(flags=1), "flags"),
]


@pytest.mark.parametrize("what,kw,word", CREATE_INVALID, ids=[w for w, _, _ in CREATE_INVALID])
def test_create_refuses_before_any_device_work(what, kw, word):
    out = C.c_void_p(0x5A5A)
    assert lib().ppf_depth_volume_create(C.byref(vparams(**kw)), C.byref(out)) == _capi.PPF_ERR_INVALID, what
    assert "ppf_depth_volume_create" in _capi.last_error() and word in _capi.last_error() and not out.value


def test_create_order_and_nulls():
    out = C.c_void_p(0x5A5A)
    assert lib().ppf_depth_volume_create(C.byref(vparams()), None) == _capi.PPF_ERR_INVALID and "out is NULL" in _capi.last_error()
    assert lib().ppf_depth_volume_create(None, C.byref(out)) == _capi.PPF_ERR_INVALID and not out.value
    order = [("dims", dict(dims=(0, 1, 1))), ("voxel", dict(voxel=-1.0)), ("origin", dict(origin=(math.nan, 0, 0))),
             ("trunc", dict(trunc=0.0)), ("max_weight", dict(max_weight=0)), ("flags", dict(flags=2))]
    for i, (word, _) in enumerate(order):     # everything from field i on is wrong: field i is named
        kw = {}
        for _, bad in order[i:]:
            kw.update(bad)
        assert lib().ppf_depth_volume_create(C.byref(vparams(**kw)), C.byref(out)) == _capi.PPF_ERR_INVALID
        assert word in _capi.last_error(), (word, _capi.last_error())
    for fn in (lib().ppf_depth_volume_reset, lib().ppf_depth_volume_release):
        assert fn(None) == (_capi.PPF_OK if fn is lib().ppf_depth_volume_release else _capi.PPF_ERR_INVALID)
    d = DepthVolumeDesc()
    C.memset(C.byref(d), 0x5A, C.sizeof(d))
    assert lib().ppf_depth_volume_info(None, C.byref(d)) == _capi.PPF_ERR_INVALID and bytes(d) == bytes(C.sizeof(d))
    rec = np.zeros(4, np.int64)
    assert lib().ppf_depth_volume_read(None, rec.ctypes.data, 4) == _capi.PPF_ERR_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="a GPU is present: volumes are created in tests/test_gpu_depth_volume.py")
def test_valid_params_reach_the_device_question():
    for kw in (dict(), dict(dims=(1, 1, 1)), dict(dims=(1024, 1024, 1024)), dict(trunc=0.004), dict(max_weight=1), dict(max_weight=65535)):
        out = C.c_void_p(0x5A5A)
        assert lib().ppf_depth_volume_create(C.byref(vparams(**kw)), C.byref(out)) == _capi.PPF_ERR_HIP, kw
        assert "no HIP device" in _capi.last_error() and not out.value


# ---- the entries on a volume ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def volume():
    """a real 8^3 volume with a device; without one a shell: a handle with the same parameters and no device memory"""
    vp = vparams(dims=(8, 8, 8), voxel=0.01, origin=(-0.035, -0.035, 0.6), trunc=0.025)
    out = C.c_void_p()
    _capi.check((lib().ppf_depth_volume_create if HAVE_GPU else lib().ppf_debug_depth_volume_shell)(C.byref(vp), C.byref(out)))
    yield out
    assert lib().ppf_depth_volume_release(out) == _capi.PPF_OK


def test_the_shell_checks_as_create_does_and_is_no_volume():
    out = C.c_void_p(0x5A5A)
    shell = lib().ppf_debug_depth_volume_shell
    assert shell(C.byref(vparams()), None) == _capi.PPF_ERR_INVALID and "out is NULL" in _capi.last_error()
    assert shell(None, C.byref(out)) == _capi.PPF_ERR_INVALID and not out.value
    for what, kw, word in CREATE_INVALID:
        out = C.c_void_p(0x5A5A)
        assert shell(C.byref(vparams(**kw)), C.byref(out)) == _capi.PPF_ERR_INVALID and word in _capi.last_error() and not out.value, what
    _capi.check(shell(C.byref(vparams(dims=(3, 4, 5))), C.byref(out)))
    try:
        d = DepthVolumeDesc()
        _capi.check(lib().ppf_depth_volume_info(out, C.byref(d)))
        assert list(d.dims) == [3, 4, 5] and d.integrations == 0 and d.device_bytes == 0 and d.max_weight == 64
        rec = np.zeros(60, np.int64)
        assert lib().ppf_depth_volume_read(out, rec.ctypes.data, 59) == _capi.PPF_ERR_INVALID and "60 voxels" in _capi.last_error()
        # where a real volume would start its device work: no device, or no volume
        want, word = (_capi.PPF_ERR_INVALID, "shell") if HAVE_GPU else (_capi.PPF_ERR_HIP, "no HIP device")
        assert lib().ppf_depth_volume_read(out, rec.ctypes.data, 60) == want and word in _capi.last_error()
        assert lib().ppf_depth_volume_reset(out) == want and word in _capi.last_error()
        assert integrate(out)[0] == want and word in _capi.last_error()
        assert integrate(out, device=True)[0] == want and raycast(out)[0] == want and raycast(out, device=True)[0] == want
        assert extract(out)[0] == want and word in _capi.last_error()
    finally:
        lib().ppf_depth_volume_release(out)


def integrate(v, device=False, depth=IMG, pitch=0, rows=ROWS, cols=COLS, intr=INTR, dp=None, pose=EYE, stats=True):
    dprm = dparams() if dp is None else dp
    it = (C.c_double * 4)(*intr) if intr is not None else None
    T = (C.c_double * 16)(*pose) if pose is not None else None
    st = DepthVolumeIntegrateStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    ptr = depth if depth is None or isinstance(depth, int) else depth.ctypes.data
    args = [v, ptr, rows, cols, pitch, it, C.byref(dprm) if dprm is not False else None, T]
    fn = lib().ppf_depth_volume_integrate_device if device else lib().ppf_depth_volume_integrate
    s = fn(*(args + ([None] if device else []) + [C.byref(st) if stats else None]))
    return s, bytes(st)


INTEGRATE_INVALID = [
    ("NULL volume", dict(v=None)),
    ("NULL pose", dict(pose=None)),
    ("NULL depth params", dict(dp=False)),
    ("NULL intr", dict(intr=None)),
    ("NULL depth", dict(depth=None)),
    ("rows 0", dict(rows=0)),
    ("cols < 0", dict(cols=-3)),
    ("too many pixels", dict(rows=1 << 16, cols=1 << 16)),
    ("unknown format", dict(dp=dparams(format=7))),
    ("pitch below the row", dict(pitch=COLS * 4 - 4)),
    ("pitch no multiple of the element", dict(pitch=COLS * 4 + 2)),
    ("misaligned", dict(depth=IMG.ctypes.data + 2)),
    ("u16 misaligned", dict(depth=IMG16.ctypes.data + 1, dp=dparams(format=_capi.PPF_DEPTH_U16))),
    ("u16 scale 0", dict(depth=IMG16, dp=dparams(format=_capi.PPF_DEPTH_U16, depth_scale=0.0))),
    ("z_min nan", dict(dp=dparams(z_min=math.nan))),
    ("z_max < 0", dict(dp=dparams(z_max=-1.0))),
    ("fx 0", dict(intr=(0.0, 20.0, 9.5, 5.5))),
    ("fy inf", dict(intr=(20.0, math.inf, 9.5, 5.5))),
    ("ppx nan", dict(intr=(20.0, 20.0, math.nan, 5.5))),
    ("pose nan", dict(pose=[math.nan] + [0.0] * 15)),
    ("pose inf", dict(pose=list(EYE[:15]) + [math.inf])),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("what,kw", INTEGRATE_INVALID, ids=[w for w, _ in INTEGRATE_INVALID])
def test_integrate_refuses_before_any_device_work(volume, what, kw, device):
    kw = dict(kw)
    v = kw.pop("v", volume)
    s, st = integrate(v, device=device, **kw)
    assert s == _capi.PPF_ERR_INVALID, (what, _capi.last_error())
    assert "ppf_depth_volume_integrate" in _capi.last_error() and st == bytes(len(st))
    assert integrate(v, device=device, stats=False, **kw)[0] == _capi.PPF_ERR_INVALID


def test_integrate_order(volume):
    integrate(None, pose=None)
    assert "volume is NULL" in _capi.last_error()
    integrate(volume, pose=None, intr=None, depth=None)
    assert "pose16 is NULL" in _capi.last_error()
    integrate(volume, intr=None, depth=None)
    assert "must not be NULL" in _capi.last_error()
    integrate(volume, pitch=2, intr=(0.0, 1.0, 0.0, 0.0))
    assert "pitch" in _capi.last_error()             # the image before the intrinsics
    integrate(volume, intr=(0.0, 1.0, 0.0, 0.0), pose=[math.nan] * 16)
    assert "fx and fy" in _capi.last_error()         # the intrinsics before the pose
    integrate(volume, pose=[math.nan] * 16)
    assert "pose16 must be finite" in _capi.last_error()


def raycast(v, device=False, rows=ROWS, cols=COLS, intr=INTR, pose=EYE, rp=None, depth=True, normals=True, stats=True):
    """one call with poisoned outputs: (status, the depth image, the normals, the stats' bytes)"""
    prm = rparams() if rp is None else rp
    it = (C.c_double * 4)(*intr) if intr is not None else None
    T = (C.c_double * 16)(*pose) if pose is not None else None
    n = max(rows, 1) * max(cols, 1) if rows * cols < 1 << 20 else 1
    d, nr = np.full(n, 7.0, np.float32), np.full(n * 3, 7.0, np.float32)
    st = DepthVolumeRaycastStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    args = [v, rows, cols, it, T, C.byref(prm) if prm is not False else None, d.ctypes.data if depth else None, nr.ctypes.data if normals else None]
    fn = lib().ppf_depth_volume_raycast_device if device else lib().ppf_depth_volume_raycast
    s = fn(*(args + ([None] if device else []) + [C.byref(st) if stats else None]))
    return s, d, nr, bytes(st)


RAYCAST_INVALID = [
    ("NULL volume", dict(v=None)),
    ("NULL depth output", dict(depth=False)),
    ("NULL pose", dict(pose=None)),
    ("NULL params", dict(rp=False)),
    ("NULL intr", dict(intr=None)),
    ("rows 0", dict(rows=0)),
    ("cols < 0", dict(cols=-1)),
    ("too many pixels", dict(rows=1 << 16, cols=1 << 16)),
    ("fx 0", dict(intr=(0.0, 20.0, 9.5, 5.5))),
    ("ppy inf", dict(intr=(20.0, 20.0, 9.5, math.inf))),
    ("pose nan", dict(pose=[0.0] * 15 + [math.nan])),
    ("z_near 0", dict(rp=rparams(z_near=0.0))),
    ("z_near nan", dict(rp=rparams(z_near=math.nan))),
    ("z_far at z_near", dict(rp=rparams(z_near=0.5, z_far=0.5))),
    ("z_far inf", dict(rp=rparams(z_far=math.inf))),
    ("ray_step 0", dict(rp=rparams(ray_step=0.0))),
    ("ray_step 1.5", dict(rp=rparams(ray_step=1.5))),
    ("ray_step nan", dict(rp=rparams(ray_step=math.nan))),
    ("min_weight 0", dict(rp=rparams(min_weight=0))),
    ("flags 4", dict(rp=rparams(flags=4))),
    ("more than 4096 steps", dict(rp=rparams(z_near=0.3, z_far=0.3 + 4096.5 * 0.0125))),   # step = 0.5 * 0.025
    ("more than 2^24 - 1 tiles", dict(rows=1, cols=(1 << 31) - 1)),     # 2^27 tiles of 16 x 16: past a launch's 2^32 lanes
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("what,kw", RAYCAST_INVALID, ids=[w for w, _ in RAYCAST_INVALID])
def test_raycast_refuses_before_any_device_work(volume, what, kw, device):
    kw = dict(kw)
    v = kw.pop("v", volume)
    s, d, nr, st = raycast(v, device=device, **kw)
    assert s == _capi.PPF_ERR_INVALID, (what, _capi.last_error())
    assert "ppf_depth_volume_raycast" in _capi.last_error() and st == bytes(len(st))
    assert (d == 7.0).all() and (nr == 7.0).all()


def test_raycast_order(volume):
    raycast(None, depth=False)
    assert "volume is NULL" in _capi.last_error()
    raycast(volume, depth=False, pose=None)
    assert "depth output is NULL" in _capi.last_error()
    raycast(volume, pose=None, rp=False)
    assert "pose16 is NULL" in _capi.last_error()
    raycast(volume, rp=False, intr=None)
    assert "raycast params are NULL" in _capi.last_error()
    raycast(volume, rows=0, intr=(0.0, 1.0, 0.0, 0.0))
    assert "the image is" in _capi.last_error()
    raycast(volume, intr=(0.0, 1.0, 0.0, 0.0), pose=[math.nan] * 16)
    assert "fx and fy" in _capi.last_error()
    raycast(volume, pose=[math.nan] * 16, rp=rparams(z_near=-1.0))
    assert "pose16 must be finite" in _capi.last_error()
    words = [("z_near", dict(z_near=-1.0)), ("ray_step", dict(ray_step=2.0)), ("min_weight", dict(min_weight=0)), ("flags", dict(flags=1))]
    for i, (word, _) in enumerate(words):
        kw = {}
        for _, bad in words[i:]:
            kw.update(bad)
        raycast(volume, rp=rparams(**kw))
        assert word in _capi.last_error(), (word, _capi.last_error())


def extract(v, ep=None, out=True, stats=True):
    prm = xparams() if ep is None else ep
    o = C.c_void_p(0x5A5A)
    st = DepthVolumeExtractStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    s = lib().ppf_depth_volume_extract(v, C.byref(prm) if prm is not False else None, C.byref(o) if out else None, C.byref(st) if stats else None)
    return s, o.value, bytes(st)


def test_extract_refuses_before_any_device_work(volume):
    for what, kw, word in [("NULL out", dict(out=False), "out is NULL"), ("NULL params", dict(ep=False), "params are NULL"),
                           ("min_weight 0", dict(ep=xparams(min_weight=0)), "min_weight"), ("flags", dict(ep=xparams(flags=8)), "flags")]:
        s, o, st = extract(volume, **kw)
        assert s == _capi.PPF_ERR_INVALID and word in _capi.last_error(), (what, _capi.last_error())
        assert st == bytes(len(st)) and (not kw.get("out", True) or not o)
    s, o, st = extract(None)
    assert s == _capi.PPF_ERR_INVALID and "volume is NULL" in _capi.last_error() and not o and st == bytes(len(st))
    extract(None, out=False)
    assert "out is NULL" in _capi.last_error()       # out before the volume
    extract(volume, ep=xparams(min_weight=0, flags=1))
    assert "min_weight" in _capi.last_error()        # min_weight before the flags


@pytest.mark.skipif(HAVE_GPU, reason="a GPU is present: the valid calls run in tests/test_gpu_depth_volume.py")
def test_valid_arguments_reach_the_device_question(volume):
    """no CPU fallback: past the argument checks a call without a device is PPF_ERR_HIP, with the outputs of a failed call"""
    for kw in (dict(), dict(depth=IMG16, dp=dparams(format=_capi.PPF_DEPTH_U16)), dict(dp=dparams(flags=0x7f)),
               dict(depth=np.zeros((ROWS, COLS + 3), np.float32), pitch=(COLS + 3) * 4), dict(rows=1, cols=1)):
        for device in (False, True):
            s, st = integrate(volume, device=device, **kw)
            assert s == _capi.PPF_ERR_HIP and "no HIP device" in _capi.last_error() and st == bytes(len(st)), kw
    ends = (dict(), dict(rp=rparams(ray_step=1.0)), dict(rp=rparams(ray_step=1e-3, z_near=0.3, z_far=0.35)), dict(rp=rparams(min_weight=65535)),
            dict(rp=rparams(z_near=0.3, z_far=0.3 + 4095.5 * 0.0125)), dict(normals=False), dict(rows=1, cols=1))
    for kw in ends:
        for device in (False, True):
            s, d, nr, st = raycast(volume, device=device, **kw)
            assert s == _capi.PPF_ERR_HIP and "no HIP device" in _capi.last_error(), (kw, _capi.last_error())
            assert (d == 7.0).all() and (nr == 7.0).all() and st == bytes(len(st))
    for kw in (dict(), dict(ep=xparams(min_weight=65535))):
        s, o, st = extract(volume, **kw)
        assert s == _capi.PPF_ERR_HIP and not o and st == bytes(len(st))
    assert lib().ppf_depth_volume_reset(volume) == _capi.PPF_ERR_HIP


FACADE_PROGRAM = r"""
#include <cstdio>
#include "ppf_cloud_stages.hpp"
int main() {
  try {
    ppf_depth_volume_params vp = ppfhip::prep::DepthVolume::defaultParams();
    vp.dims[0] = vp.dims[1] = vp.dims[2] = 8;
    vp.voxel = 0.01f; vp.trunc = 0.025f;
    vp.origin[0] = vp.origin[1] = -0.035; vp.origin[2] = 0.6;
    ppfhip::prep::DepthVolume vol(vp);
    const double intr[4] = {20.0, 20.0, 9.5, 5.5};
    const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<float> img(12 * 20, 0.64f);
    std::vector<uint16_t> img16(12 * 20, 642);
    const ppf_depth_volume_integrate_stats a = vol.integrate(&img[0], 12, 20, intr, eye);
    const ppf_depth_volume_integrate_stats b = vol.integrateU16(&img16[0], 12, 20, 0.001, intr, eye);
    ppf_depth_volume_raycast_params rp;
    ppf_default_depth_volume_raycast_params(&rp);
    rp.z_near = 0.5f; rp.z_far = 0.8f;
    std::vector<float> normals;
    ppf_depth_volume_raycast_stats rs;
    const std::vector<float> depth = vol.raycast(12, 20, intr, eye, &rp, &normals, &rs);
    ppf_depth_volume_extract_stats xs;
    const ppfhip::prep::Cloud cloud = vol.extract(0, &xs);
    const std::vector<ppf_depth_volume_voxel> vox = vol.read();
    long long w = 0;
    for (size_t i = 0; i < vox.size(); i++) w += vox[i].w;
    std::printf("%lld %lld %d %d %lld %lld %d %lld %zu %zu %lld\n", (long long)a.n_updated, (long long)b.n_updated, rs.n_hits, rs.n_interpolated,
                (long long)xs.n_crossings, (long long)xs.n_rows, cloud.size(), w, depth.size(), normals.size(), (long long)vol.info().integrations);
    vol.reset();
    return 0;
  } catch (const ppfhip::ppf_match_3d::Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 10 + (int)e.status;
  }
}
"""


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_the_cxx_facade_compiles_as_cxx11_and_runs(tmp_path, compiler):
    """prep::DepthVolume, warnings as errors; without a device the program ends with PPF_ERR_HIP's exit code, with one its
    counts are the oracle's"""
    csrc = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
    src = tmp_path / "volume_facade.cpp"
    src.write_text(FACADE_PROGRAM)
    exe = str(tmp_path / "volume_facade")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", csrc,
                    "-lppf_hip", f"-Wl,-rpath,{csrc}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    if not HAVE_GPU:
        assert r.returncode == 10 + _capi.PPF_ERR_HIP and "no HIP device" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    import depth_volume_oracle as O
    ov = O.Volume((8, 8, 8), 0.01, (-0.035, -0.035, 0.6), trunc=0.025)
    a = O.integrate(ov, np.full((12, 20), 0.64, np.float32), INTR, np.eye(4))
    b = O.integrate(ov, np.full((12, 20), 642, np.uint16), INTR, np.eye(4))
    depth, normals, rs = O.raycast(ov, (12, 20), INTR, np.eye(4), z_near=0.5, z_far=0.8, normals=True)
    rows, xs = O.extract(ov)
    want = [a, b, rs["n_hits"], rs["n_interpolated"], xs["n_crossings"], xs["n_rows"], len(rows), int(ov.w.sum()), 240, 720, 2]
    assert [int(v) for v in r.stdout.split()] == want


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_the_demo_is_cxx11(tmp_path, compiler):
    """examples/depth_volume_demo.cpp and the facade behind it, warnings as errors; a file it cannot read is its own exit code"""
    csrc = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
    exe = str(tmp_path / "depth_volume_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "depth_volume_demo.cpp"), "-L", csrc, "-lppf_hip", f"-Wl,-rpath,{csrc}", "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True).returncode == 1
    r = subprocess.run([exe, str(tmp_path / "missing.f32"), "2", "4", "4", "1", "1", "0", "0", "8", "8", "8", "0.01", "0", "0", "0.5", "0.03"],
                       capture_output=True, text=True)
    assert r.returncode == 10 + _capi.PPF_ERR_IO and "cannot read" in r.stderr


def test_python_wrappers_check_their_arguments():
    from yolo_ppf_pose_estimation_amd.cloud_processor import DepthVolume
    with pytest.raises(_capi.PPFError) as e:
        DepthVolume((8, 8), 0.01, (0, 0, 0.5))
    assert e.value.status == _capi.PPF_ERR_INVALID and "dims" in str(e.value)
    with pytest.raises(_capi.PPFError) as e:
        DepthVolume((8, 8, 0), 0.01, (0, 0, 0.5))
    assert e.value.status == _capi.PPF_ERR_INVALID and "dims[2]" in str(e.value)
    with pytest.raises(_capi.PPFError) as e:
        DepthVolume((8, 8, 8), 0.01, (0, 0, 0.5), trunc=0.001)
    assert "trunc" in str(e.value)
    if not HAVE_GPU:
        with pytest.raises(_capi.PPFError) as e:
            DepthVolume((8, 8, 8), 0.01, (0, 0, 0.5))      # trunc None: 4 voxels, valid
        assert e.value.status == _capi.PPF_ERR_HIP
