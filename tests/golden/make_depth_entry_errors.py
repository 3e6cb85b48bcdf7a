"""Regenerate tests/golden/depth_entry_errors.json: the argument-error contract of the depth-image entries, byte for byte.

Recorded with the library of commit d3cac5cb8508fed55b78d0c6b16849d5d5ecf550 ("Add ppf_depth_history"), before the
depth-image stages were moved onto one shared host front end, on a machine without a GPU.  It is NOT regenerated when that code moves: the point of
the file is that every status, every ppf_last_error() text and which of two errors wins stay what they were.

    python tests/golden/make_depth_entry_errors.py        (CPU only; a second)

For the 11 entries that take a depth image and for ppf_depth_history_create, cases() is a table of calls through ctypes.  Of
each call the file keeps the status, the whole error text and what came back: whether the stats are zero, and what happened
to the outputs (the cloud handle NULL, counts and info zero, the output image untouched).  Device entries get pointers that
are never dereferenced.  ppf_depth_map_create and ppf_depth_history_create need a device, so without one the register and
push entries can only be called with a NULL handle: their later checks are pinned by tests/test_gpu_register.py,
tests/test_gpu_depth_history.py and tests/test_gpu_depth_front_end.py.  The one fully valid call of each entry ends in
"no HIP device" here; where a device is present tests/test_depth_entry_errors.py does not make those calls."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from yolo_ppf_pose_estimation_amd import _capi  # noqa: E402
from yolo_ppf_pose_estimation_amd._capi import (DepthFilterParams, DepthFilterStats, DepthHistoryParams, DepthHistoryStats,  # noqa: E402
                                                DepthNormalParams, DepthParams, RegisterParams, RegisterStats, SegmentInfo,
                                                SegmentParams, SegmentStats, lib)

OUT = os.path.join(HERE, "depth_entry_errors.json")
SENTINEL = 0x5A5A5A5A
INTR = (500.0, 500.0, 3.0, 2.0)
U16 = _capi.PPF_DEPTH_U16
BELOW0 = float(np.nextafter(np.float32(0), np.float32(-1)))     # one float step under 0
ABOVE1 = float(np.nextafter(np.float32(1), np.float32(2)))
HUGE_PITCH = 1 << 63
MAX_PITCH = (1 << 64) - 1                                        # SIZE_MAX: a pitch like any other, odd and too large
VALID = "valid"                                                  # the name of each entry's fully valid call


def _made(cls, default, **kw):
    p = cls()
    getattr(lib(), default)(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def dp(**kw):
    return _made(DepthParams, "ppf_default_depth_params", **kw)


def nprm(**kw):
    return _made(DepthNormalParams, "ppf_default_depth_normal_params", **kw)


def fprm(**kw):
    return _made(DepthFilterParams, "ppf_default_depth_filter_params", **kw)


def sprm(**kw):
    return _made(SegmentParams, "ppf_default_segment_params", **kw)


def rprm(**kw):
    return _made(RegisterParams, "ppf_default_register_params", **kw)


def hprm(**kw):
    return _made(DepthHistoryParams, "ppf_default_depth_history_params", **kw)


def _ref(p):
    return None if p is False else C.byref(p)


def _dirty(cls):
    st = cls()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    return st


def _zero(rec):
    return bytes(rec) == bytes(C.sizeof(rec))


class Image:
    """the image argument of a call: a host array for the host entry, a pointer that is never read for the device entry"""

    def __init__(self, device, kind="f32"):
        self.keep = None
        if kind is None:
            self.ptr = None
        elif device:
            self.ptr = C.c_void_p(0x11 if kind == "odd" else 0x10)
        else:
            self.keep = np.zeros(64, np.uint8)[1:] if kind == "odd" else np.zeros((4, 6), np.uint16 if kind == "u16" else np.float32)
            self.ptr = C.c_void_p(self.keep.ctypes.data)


def call_cloud(device, normals, img="f32", rows=4, cols=6, pitch=0, intr=INTR, p=None, np_=None, out=True):
    im = Image(device, img)
    it = (C.c_double * 4)(*intr) if intr is not None else None
    o = C.c_void_p(SENTINEL)
    args = [im.ptr, rows, cols, pitch, it, _ref(dp() if p is None else p)]
    if normals:
        args.append(_ref(nprm() if np_ is None else np_))
    if device:
        args.append(None)
    name = "ppf_cloud_from_depth" + ("_normals" if normals else "") + ("_device" if device else "")
    s = getattr(lib(), name)(*args, C.byref(o) if out else None)
    return s, {"out": "NULL" if o.value is None else "untouched"}


def call_filter(device, img="f32", rows=4, cols=6, pitch=0, p=None, fp=None, out=True, stats=True):
    im = Image(device, img)
    res = np.full((4, 6), np.float32(7.0))
    st = _dirty(DepthFilterStats)
    optr = None if not out else C.c_void_p(0x100000) if device else C.c_void_p(res.ctypes.data)
    args = [im.ptr, rows, cols, pitch, _ref(dp() if p is None else p), _ref(fprm() if fp is None else fp), optr]
    if device:
        args.append(None)
    s = getattr(lib(), "ppf_depth_filter" + ("_device" if device else ""))(*args, C.byref(st) if stats else None)
    return s, {"stats_zero": _zero(st) if stats else None, "out": "untouched" if (res == 7.0).all() else "written"}


def call_segments(device, img="f32", rows=4, cols=6, pitch=0, p=None, sp=None, labels=True, info=True, counts=True, stats=True):
    im = Image(device, img)
    sp = sprm() if sp is None else sp
    lab = np.full((4, 6), 7, np.int32)
    inf = (SegmentInfo * 256)()
    C.memset(inf, 0x5A, C.sizeof(inf))
    cnt = (C.c_int32 * 3)(7, 7, 7)
    st = _dirty(SegmentStats)
    lptr = None if not labels else C.c_void_p(labels if labels is not True else 0x100000) if device else C.c_void_p(lab.ctypes.data)
    args = [im.ptr, rows, cols, pitch, _ref(dp() if p is None else p), None, _ref(sp), lptr]
    if device:
        args.append(None)
    s = getattr(lib(), "ppf_depth_segments" + ("_device" if device else ""))(*args, inf if info else None, cnt if counts else None,
                                                                            C.byref(st) if stats else None)
    shown = sp.max_segments if sp is not False and 1 <= sp.max_segments <= 256 else 0
    raw = bytes(inf)
    return s, {"stats_zero": _zero(st) if stats else None, "counts": list(cnt),
               "info_zeroed_records": shown if raw[:shown * C.sizeof(SegmentInfo)] == bytes(shown * C.sizeof(SegmentInfo)) else -1,
               "info_rest_untouched": raw[shown * C.sizeof(SegmentInfo):] == b"\x5a" * (len(raw) - shown * C.sizeof(SegmentInfo)),
               "labels": "untouched" if (lab == 7).all() else "written"}


def call_register(device, img="f32", pitch=0, p=None, rp=None, out=True, stats=True):
    """without a device there is no map: every call goes in with a NULL one"""
    im = Image(device, img)
    res = np.full((4, 6), np.float32(7.0))
    st = _dirty(RegisterStats)
    optr = None if not out else C.c_void_p(0x100000) if device else C.c_void_p(res.ctypes.data)
    args = [None, im.ptr, pitch, _ref(dp() if p is None else p), _ref(rprm() if rp is None else rp), optr]
    if device:
        args.append(None)
    s = getattr(lib(), "ppf_depth_register" + ("_device" if device else ""))(*args, C.byref(st) if stats else None)
    return s, {"stats_zero": _zero(st) if stats else None, "out": "untouched" if (res == 7.0).all() else "written"}


def call_push(device, img="f32", pitch=0, out=True, state=True, stats=True):
    """without a device there is no history: every call goes in with a NULL one"""
    im = Image(device, img)
    res, sta = np.full((4, 6), np.float32(7.0)), np.full((4, 6), 7, np.uint8)
    st = _dirty(DepthHistoryStats)
    optr = None if not out else C.c_void_p(0x100000) if device else C.c_void_p(res.ctypes.data)
    sptr = None if not state else C.c_void_p(0x200000) if device else C.c_void_p(sta.ctypes.data)
    args = [None, im.ptr, pitch, optr, sptr]
    if device:
        args.append(None)
    s = getattr(lib(), "ppf_depth_history_push" + ("_device" if device else ""))(*args, C.byref(st) if stats else None)
    return s, {"stats_zero": _zero(st) if stats else None,
               "out": "untouched" if (res == 7.0).all() and (sta == 7).all() else "written"}


def call_create(rows=4, cols=6, p=None, hp=None, out=True):
    h = C.c_void_p(SENTINEL)
    s = lib().ppf_depth_history_create(rows, cols, _ref(dp() if p is None else p), _ref(hprm() if hp is None else hp),
                                       C.byref(h) if out else None)
    return s, {"out": "NULL" if h.value is None else "untouched"}


def image_cases():
    """what every entry with an image checks"""
    c = [
        ("NULL depth", dict(img=None)),
        ("NULL depth params", dict(p=False)),
        ("rows 0", dict(rows=0)),
        ("cols -1", dict(cols=-1)),
        ("rows * cols > INT32_MAX", dict(rows=65536, cols=32768)),
        ("format 2", dict(p=dp(format=2))),
        ("format -1", dict(p=dp(format=-1))),
        ("pitch below the width", dict(pitch=20)),
        ("pitch no multiple of the element", dict(pitch=26)),
        ("pitch no multiple of the element, u16", dict(img="u16", pitch=13, p=dp(format=U16))),
        ("pitch too large", dict(pitch=HUGE_PITCH)),
        ("pitch SIZE_MAX", dict(pitch=MAX_PITCH)),
        ("pitch SIZE_MAX, u16", dict(img="u16", pitch=MAX_PITCH, p=dp(format=U16))),
        ("pitch SIZE_MAX - 3", dict(pitch=MAX_PITCH - 3)),
        ("pitch SIZE_MAX + NULL depth", dict(img=None, pitch=MAX_PITCH)),
        ("pitch SIZE_MAX + misaligned", dict(img="odd", pitch=MAX_PITCH)),
        ("pitch SIZE_MAX + z_max -1", dict(pitch=MAX_PITCH, p=dp(z_max=-1.0))),
        ("pitch one row wider", dict(pitch=48)),                       # valid
        ("misaligned f32", dict(img="odd")),
        ("misaligned u16", dict(img="odd", p=dp(format=U16))),
        ("u16 scale 0", dict(img="u16", p=dp(format=U16, depth_scale=0.0))),
        ("u16 scale inf", dict(img="u16", p=dp(format=U16, depth_scale=math.inf))),
        ("f32 scale 0", dict(p=dp(depth_scale=0.0))),                  # valid: the scale is U16's
        ("z_min nan", dict(p=dp(z_min=math.nan))),
        ("z_min inf", dict(p=dp(z_min=math.inf))),
        ("z_max -1", dict(p=dp(z_max=-1.0))),
        ("z_max just below 0", dict(p=dp(z_max=BELOW0))),
        ("flags FP64", dict(p=dp(flags=_capi.PPF_DEPTH_FP64))),
        ("flags 2", dict(p=dp(flags=2))),
        # two at once, inside the image checks
        ("rows 0 + format 2", dict(rows=0, p=dp(format=2))),
        ("format 2 + flags 2", dict(p=dp(format=2, flags=2))),
        ("flags 2 + pitch below", dict(p=dp(flags=2), pitch=20)),
        ("pitch below + misaligned", dict(img="odd", pitch=20)),
        ("misaligned + u16 scale 0", dict(img="odd", p=dp(format=U16, depth_scale=0.0))),
        ("u16 scale 0 + z_min nan", dict(img="u16", p=dp(format=U16, depth_scale=0.0, z_min=math.nan))),
        ("NULL depth + NULL depth params + rows 0", dict(img=None, p=False, rows=0)),
    ]
    return c


def cloud_cases(normals):
    c = image_cases() + [
        ("NULL out", dict(out=False)),
        ("NULL intr", dict(intr=None)),
        ("fx 0", dict(intr=(0.0, 500.0, 3.0, 2.0))),
        ("fy inf", dict(intr=(500.0, math.inf, 3.0, 2.0))),
        ("ppx nan", dict(intr=(500.0, 500.0, math.nan, 2.0))),
        ("ppy inf", dict(intr=(500.0, 500.0, 3.0, math.inf))),
        ("NULL out + NULL depth", dict(out=False, img=None)),
        ("NULL intr + rows 0", dict(intr=None, rows=0)),
        ("u16 scale 0 + fx 0", dict(img="u16", p=dp(format=U16, depth_scale=0.0), intr=(0.0, 500.0, 3.0, 2.0))),
        ("misaligned + fx 0", dict(img="odd", intr=(0.0, 500.0, 3.0, 2.0))),
        ("fx 0 + ppx nan", dict(intr=(0.0, 500.0, math.nan, 2.0))),
        ("fx 0 + z_min nan", dict(intr=(0.0, 500.0, 3.0, 2.0), p=dp(z_min=math.nan))),
        ("ppx nan + z_max -1", dict(intr=(500.0, 500.0, math.nan, 2.0), p=dp(z_max=-1.0))),
        (VALID, dict()),
    ]
    if normals:
        c += [
            ("NULL normal params", dict(np_=False)),
            ("radius 0", dict(np_=nprm(radius=0))),
            ("radius 9", dict(np_=nprm(radius=9))),
            ("radius 8", dict(np_=nprm(radius=8))),                    # valid
            ("max_depth_change 0", dict(np_=nprm(max_depth_change=0.0))),
            ("max_depth_change inf", dict(np_=nprm(max_depth_change=math.inf))),
            ("min_neighbours 2", dict(np_=nprm(min_neighbours=2))),
            ("min_neighbours 50 of 49", dict(np_=nprm(radius=3, min_neighbours=50))),
            ("min_neighbours 49 of 49", dict(np_=nprm(radius=3, min_neighbours=49))),   # valid
            ("normal flags 2", dict(np_=nprm(flags=2))),
            ("NULL normal params + z_max -1", dict(np_=False, p=dp(z_max=-1.0))),
            ("radius 0 + ppx nan", dict(np_=nprm(radius=0), intr=(500.0, 500.0, math.nan, 2.0))),
            ("radius 0 + NULL out", dict(np_=nprm(radius=0), out=False)),
            ("radius 9 + min_neighbours 2", dict(np_=nprm(radius=9, min_neighbours=2))),
        ]
    return c


def filter_cases():
    return image_cases() + [
        ("NULL out", dict(out=False)),
        ("NULL filter params", dict(fp=False)),
        ("NULL stats", dict(stats=False, rows=0)),
        ("radius -1", dict(fp=fprm(radius=-1))),
        ("radius 9", dict(fp=fprm(radius=9))),
        ("radius 0", dict(fp=fprm(radius=0))),                         # valid
        ("range_abs 0", dict(fp=fprm(range_abs=0.0))),
        ("range_abs inf", dict(fp=fprm(range_abs=math.inf))),
        ("range_quad below 0", dict(fp=fprm(range_quad=BELOW0))),
        ("support_abs below 0", dict(fp=fprm(support_abs=BELOW0))),
        ("support_quad nan", dict(fp=fprm(support_quad=math.nan))),
        ("min_support -1", dict(fp=fprm(min_support=-1))),
        ("min_support 9", dict(fp=fprm(min_support=9))),
        ("filter flags 1", dict(fp=fprm(flags=1))),
        ("NULL out + rows 0", dict(out=False, rows=0)),
        ("NULL out + NULL filter params", dict(out=False, fp=False)),
        ("NULL filter params + format 2", dict(fp=False, p=dp(format=2))),
        ("radius 9 + z_min nan", dict(fp=fprm(radius=9), p=dp(z_min=math.nan))),
        ("radius 9 + NULL depth", dict(fp=fprm(radius=9), img=None)),
        ("radius 9 + range_abs 0", dict(fp=fprm(radius=9, range_abs=0.0))),
        (VALID, dict()),
    ]


def segment_cases(device):
    c = image_cases() + [
        ("NULL labels", dict(labels=False)),
        ("NULL info", dict(info=False)),
        ("NULL counts", dict(counts=False)),
        ("NULL segment params", dict(sp=False)),
        ("NULL stats", dict(stats=False, rows=0)),
        ("depth_abs below 0", dict(sp=sprm(depth_abs=BELOW0))),
        ("depth_quad inf", dict(sp=sprm(depth_quad=math.inf))),
        ("normal_cos above 1", dict(sp=sprm(normal_cos=ABOVE1))),
        ("normal_cos below -1", dict(sp=sprm(normal_cos=-ABOVE1))),
        ("normal_cos 1", dict(sp=sprm(normal_cos=1.0))),               # valid
        ("curvature_threshold below 0", dict(sp=sprm(curvature_threshold=BELOW0))),
        ("curvature_threshold nan", dict(sp=sprm(curvature_threshold=math.nan))),
        ("min_size 0", dict(sp=sprm(min_size=0))),
        ("max_size -1", dict(sp=sprm(max_size=-1))),
        ("max_segments 0", dict(sp=sprm(max_segments=0))),
        ("max_segments 257", dict(sp=sprm(max_segments=257))),
        ("max_segments 256", dict(sp=sprm(max_segments=256))),         # valid
        ("segment flags 4", dict(sp=sprm(flags=4))),
        ("NULL labels + pitch below", dict(labels=False, pitch=20)),
        ("NULL segment params + format 2", dict(sp=False, p=dp(format=2))),
        ("NULL counts + NULL segment params", dict(counts=False, sp=False)),
        ("min_size 0 + z_max -1", dict(sp=sprm(min_size=0), p=dp(z_max=-1.0))),
        ("min_size 0 + rows 0", dict(sp=sprm(min_size=0, max_segments=3), rows=0)),
        ("max_segments 0 + NULL depth", dict(sp=sprm(max_segments=0), img=None)),
        (VALID, dict()),
    ]
    if device:
        c += [
            ("misaligned labels", dict(labels=0x100002)),
            ("misaligned labels + segment flags 4", dict(labels=0x100002, sp=sprm(flags=4))),
            ("misaligned labels + z_min nan", dict(labels=0x100002, p=dp(z_min=math.nan))),
        ]
    return c


def register_cases():
    return [
        ("NULL map", dict()),
        ("NULL map + NULL out", dict(out=False)),
        ("NULL map + NULL register params", dict(rp=False)),
        ("NULL map + depth flags 1", dict(p=dp(flags=1))),
        ("NULL map + NULL depth", dict(img=None)),
        ("NULL map + NULL depth params", dict(p=False)),
        ("NULL map + format 2", dict(p=dp(format=2))),
        ("NULL map + pitch SIZE_MAX", dict(pitch=MAX_PITCH)),
        ("NULL map + quad_dz_abs below 0", dict(rp=rprm(quad_dz_abs=BELOW0))),
        ("NULL map + register flags 1", dict(rp=rprm(flags=1))),
        ("NULL map + NULL stats", dict(stats=False)),
    ]


def push_cases():
    return [
        ("NULL history", dict()),
        ("NULL history + NULL out", dict(out=False)),
        ("NULL history + NULL state", dict(state=False)),
        ("NULL history + NULL depth", dict(img=None)),
        ("NULL history + pitch below", dict(pitch=20)),
        ("NULL history + pitch SIZE_MAX", dict(pitch=MAX_PITCH)),
        ("NULL history + NULL stats", dict(stats=False)),
    ]


def create_cases():
    return [
        ("NULL out", dict(out=False)),
        ("NULL history params", dict(hp=False)),
        ("NULL depth params", dict(p=False)),
        ("rows 0", dict(rows=0)),
        ("cols -1", dict(cols=-1)),
        ("rows * cols > INT32_MAX", dict(rows=65536, cols=32768)),
        ("format 2", dict(p=dp(format=2))),
        ("u16 scale 0", dict(p=dp(format=U16, depth_scale=0.0))),
        ("u16 scale inf", dict(p=dp(format=U16, depth_scale=math.inf))),
        ("z_min nan", dict(p=dp(z_min=math.nan))),
        ("z_max -1", dict(p=dp(z_max=-1.0))),
        ("flags FP64", dict(p=dp(flags=_capi.PPF_DEPTH_FP64))),       # valid: ignored
        ("flags 6", dict(p=dp(flags=6))),                              # valid: ignored
        ("window 0", dict(hp=hprm(window=0))),
        ("window 17", dict(hp=hprm(window=17))),
        ("window 16", dict(hp=hprm(window=16))),                       # valid
        ("range_abs 0", dict(hp=hprm(range_abs=0.0))),
        ("range_quad below 0", dict(hp=hprm(range_quad=BELOW0))),
        ("min_support 0", dict(hp=hprm(min_support=0))),
        ("min_support window + 1", dict(hp=hprm(window=5, min_support=6))),
        ("max_age -1", dict(hp=hprm(max_age=-1))),
        ("max_age 16", dict(hp=hprm(max_age=16))),
        ("history flags 2", dict(hp=hprm(flags=2))),
        ("NULL out + NULL history params", dict(out=False, hp=False)),
        ("NULL history params + rows 0", dict(hp=False, rows=0)),
        ("NULL depth params + rows 0", dict(p=False, rows=0)),
        ("window 0 + format 2", dict(hp=hprm(window=0), p=dp(format=2))),
        ("window 0 + z_max -1", dict(hp=hprm(window=0), p=dp(z_max=-1.0))),
        ("rows 0 + u16 scale 0", dict(rows=0, p=dp(format=U16, depth_scale=0.0))),
        ("window 17 + min_support 0", dict(hp=hprm(window=17, min_support=0))),
        (VALID, dict()),
    ]


def cases():
    """[(entry, case name, the call)], in a fixed order"""
    table = []
    for device in (False, True):
        sfx = "_device" if device else ""
        for normals in (False, True):
            name = "ppf_cloud_from_depth" + ("_normals" if normals else "") + sfx
            table += [(name, n, lambda kw=kw, d=device, nm=normals: call_cloud(d, nm, **kw)) for n, kw in cloud_cases(normals)]
        table += [("ppf_depth_register" + sfx, n, lambda kw=kw, d=device: call_register(d, **kw)) for n, kw in register_cases()]
        table += [("ppf_depth_filter" + sfx, n, lambda kw=kw, d=device: call_filter(d, **kw)) for n, kw in filter_cases()]
        table += [("ppf_depth_segments" + sfx, n, lambda kw=kw, d=device: call_segments(d, **kw)) for n, kw in segment_cases(device)]
        table += [("ppf_depth_history_push" + sfx, n, lambda kw=kw, d=device: call_push(d, **kw)) for n, kw in push_cases()]
    table += [("ppf_depth_history_create", n, lambda kw=kw: call_create(**kw)) for n, kw in create_cases()]
    return table


def replay(wanted=lambda entry, name: True):
    """{entry: {case: [status, error, after]}} of the calls that `wanted` picks, made in the table's order; every error text
    begins with "<entry>: ", which is left out of the record"""
    got = {}
    for entry, name, fn in cases():
        if not wanted(entry, name):
            continue
        s, after = fn()
        assert name not in got.setdefault(entry, {}), (entry, name)
        err = _capi.last_error() if s != _capi.PPF_OK else entry + ": "
        assert err.startswith(entry + ": "), (entry, name, err)
        got[entry][name] = [_capi.STATUS_NAMES[s], err[len(entry) + 2:], after]
    return got


if __name__ == "__main__":
    assert lib().ppf_device_count() == 0, "record on a machine without a GPU: the valid calls must end in 'no HIP device'"
    rec = replay()
    with open(OUT, "w") as f:                                     # one line per call
        f.write("{\n" + ",\n".join(json.dumps(e) + ": {\n" + ",\n".join(f" {json.dumps(n)}: {json.dumps(c, sort_keys=True)}"
                                                                      for n, c in sorted(v.items())) + "\n}"
                                   for e, v in sorted(rec.items())) + "\n}\n")
    n = sum(len(v) for v in rec.values())
    print(f"{OUT}: {len(rec)} entries, {n} calls, {os.path.getsize(OUT)} bytes")
