"""ppf_match_frame's C-ABI surface without a GPU: the two structs as a C compiler lays them out equal their ctypes
mirrors, argument errors come before any device work (and leave n_out zero), and the call fails loudly (PPF_ERR_HIP)
when there is no device."""
import ctypes as C
import os
import subprocess

import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import FrameDetection, IcpParams, MatchFrameStats, MatchParams, Pose, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_match_frame_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "msz.c"
    fields_d = ["model", "model_cloud", "scene", "edge"]
    fields_s = ["n_dets", "n_matched", "n_icp_jobs", "n_icp_launches", "n_icp_passes", "n_host_syncs", "ms_wall", "ms_match",
                "ms_icp", "reserved"]
    expr = ["sizeof(ppf_frame_detection)"] + [f"offsetof(ppf_frame_detection, {f})" for f in fields_d] + \
           ["sizeof(ppf_match_frame_stats)"] + [f"offsetof(ppf_match_frame_stats, {f})" for f in fields_s]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppf_hip.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "msz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    got = [C.sizeof(FrameDetection)] + [getattr(FrameDetection, f).offset for f in fields_d] + \
          [C.sizeof(MatchFrameStats)] + [getattr(MatchFrameStats, f).offset for f in fields_s]
    assert got == want


def _params():
    mp, ip = MatchParams(), IcpParams()
    lib().ppf_default_match_params(C.byref(mp))
    lib().ppf_default_icp_params(C.byref(ip))
    mp.relative_scene_sample_step, mp.relative_scene_distance = 0.05, 0.05
    return mp, ip


def _call(dets, n_dets, top=5, out=True, n_out=True, mp=None, ip=None):
    d_mp, d_ip = _params()
    mp = d_mp if mp is None else mp
    ip = d_ip if ip is None else ip
    cap = max(n_dets, 1)
    poses = (Pose * (cap * 16))() if out else None
    counts = (C.c_int * 300)(*([77] * 300)) if n_out else None   # garbage the call must overwrite
    st = MatchFrameStats()
    st.n_icp_launches = 99
    s = lib().ppf_match_frame(dets, n_dets, C.byref(mp), C.byref(ip), top, poses, counts, None, C.byref(st))
    return s, counts, st


def _dets(n, scene=True):
    dummy = C.create_string_buffer(64)   # never dereferenced: every check below fails before a handle is used
    arr = (FrameDetection * 300)()
    for i in range(n):
        arr[i].model = C.addressof(dummy)
        arr[i].model_cloud = C.addressof(dummy)
        arr[i].scene = C.addressof(dummy) if scene else None
    arr._keep = dummy
    return arr


def test_argument_errors_precede_any_device_work():
    dets = _dets(3)
    s, counts, st = _call(dets, 257)
    assert s == _capi.PPF_ERR_INVALID and "n_dets" in _capi.last_error()
    assert _call(dets, -1)[0] == _capi.PPF_ERR_INVALID
    for top in (0, 17, -3):
        s, counts, _ = _call(dets, 3, top=top)
        assert s == _capi.PPF_ERR_INVALID and "top" in _capi.last_error()
        assert list(counts[:3]) == [0, 0, 0] and counts[3] == 77   # n_out zeroed, nothing beyond n_dets touched
    assert _call(dets, 3, out=False)[0] == _capi.PPF_ERR_INVALID
    assert _call(dets, 3, n_out=False)[0] == _capi.PPF_ERR_INVALID
    assert lib().ppf_match_frame(None, 2, C.byref(_params()[0]), C.byref(_params()[1]), 5, (Pose * 32)(), (C.c_int * 2)(), None,
                                 None) == _capi.PPF_ERR_INVALID
    # a detection with a model but no scene
    bad = _dets(3)
    bad[1].scene = None
    s, counts, st = _call(bad, 3)
    assert s == _capi.PPF_ERR_INVALID and "detection 1" in _capi.last_error()
    assert list(counts[:3]) == [0, 0, 0]
    assert st.n_icp_launches == 0 and st.n_host_syncs == 0
    # bad match / ICP parameters
    mp, ip = _params()
    mp.relative_scene_sample_step = 0.0
    assert _call(dets, 3, mp=mp)[0] == _capi.PPF_ERR_INVALID
    mp, ip = _params()
    ip.num_levels = -1
    assert _call(dets, 3, ip=ip)[0] == _capi.PPF_ERR_INVALID


def test_skipped_detections_need_no_scene():
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    dets = (FrameDetection * 4)()   # all NULL: every detection skipped; the arguments are valid
    s, counts, st = _call(dets, 4)
    assert s == _capi.PPF_ERR_HIP and list(counts[:4]) == [0, 0, 0, 0]


def test_match_frame_without_a_device_is_loud():
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    for n in (0, 3):
        s, counts, st = _call(_dets(n), n)
        assert s == _capi.PPF_ERR_HIP
        assert "no HIP device" in _capi.last_error() and "ppf_match_frame" in _capi.last_error()
        assert list(counts[:n]) == [0] * n
        assert st.n_icp_launches == 0 and st.n_host_syncs == 0
