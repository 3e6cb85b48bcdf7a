"""The C-ABI library loads without a GPU, exports every symbol include/ppf_hip.h declares, and its
host-only entry points behave (no compute calls here; compute parity lives in the -m gpu tests)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import MatchParams, TrainParams, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    text = open(os.path.join(ROOT, "include", "ppf_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ppf_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound():
    names = _header_functions()
    assert len(names) >= 25
    L = C.CDLL(_capi.LIB_PATH)
    for n in names:
        assert hasattr(L, n), f"libppf_hip.so lacks {n}"
    assert sorted(_capi._SIGNATURES) == names, "python binding table and header disagree"
    assert lib().ppf_abi_version() == _capi.PPF_ABI_VERSION == 4


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof() of every struct as a C compiler sees include/ppf_hip.h == the ctypes mirror."""
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppf_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(ppf_pose),sizeof(ppf_vote),sizeof(ppf_train_params),sizeof(ppf_match_params),'
                   'sizeof(ppf_model_info),sizeof(ppf_match_stats),sizeof(ppf_batch_stats),'
                   'offsetof(ppf_match_stats, n_lds_atomics),offsetof(ppf_match_params, vote_mode),'
                   'sizeof(ppf_debug_pool_violation),sizeof(ppf_debug_pool_report),offsetof(ppf_debug_pool_report, first));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    got = [C.sizeof(t) for t in (_capi.Pose, _capi.Vote, TrainParams, MatchParams, _capi.ModelInfo, _capi.MatchStats,
                                 _capi.BatchStats)] + [_capi.MatchStats.n_lds_atomics.offset, MatchParams.vote_mode.offset,
                                                     C.sizeof(_capi.PoolViolation), C.sizeof(_capi.PoolReport), _capi.PoolReport.first.offset]
    assert got == want


def test_defaults_mirror_the_reference_library():
    tp, mp = TrainParams(), MatchParams()
    lib().ppf_default_train_params(C.byref(tp))
    lib().ppf_default_match_params(C.byref(mp))
    assert (tp.relative_sampling_step, tp.relative_distance_step, tp.num_angles) == (0.05, 0.05, 30)
    assert mp.relative_scene_sample_step == pytest.approx(0.2) and mp.relative_scene_distance == 0.03
    assert mp.position_threshold < 0 and mp.rotation_threshold < 0 and mp.ref_stride == 1


def test_errors_without_a_device_are_loud(bottle):
    """No CPU fallback: on a box without a GPU every compute entry point reports PPF_ERR_HIP."""
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    from yolo_ppf_pose_estimation_amd.detector import ICP, PPF3DDetector, samplePCByQuantization, transformPCPose
    calls = [lambda: PPF3DDetector(0.05, 0.05).trainModel(bottle),
             lambda: samplePCByQuantization(bottle, 0.05),
             lambda: transformPCPose(bottle[:10], np.eye(4)),
             lambda: ICP().registerModelToScene(bottle[:100], bottle[:100]),
             lambda: ICP().registerModelToScene(bottle[:100], bottle[:100], [])]
    for call in calls:
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_HIP
        assert "no HIP device" in str(e.value)


def test_argument_validation_precedes_any_device_work(bottle):
    from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
    det = PPF3DDetector(0.05, 0.05)
    with pytest.raises(_capi.PPFError) as e:
        det.match(bottle[:100])
    assert e.value.status == _capi.PPF_ERR_NOT_TRAINED  # the wrapper's pre-check, CloudProcessing.h:435-439
    with pytest.raises(_capi.PPFError) as e:
        det.trainModel(bottle[:, :3])
    assert e.value.status == _capi.PPF_ERR_INVALID
    out = C.c_void_p()
    tp = TrainParams()
    lib().ppf_default_train_params(C.byref(tp))
    assert lib().ppf_model_train(None, 10, 6, 3, C.byref(tp), C.byref(out)) == _capi.PPF_ERR_INVALID
    assert "bad argument" in _capi.last_error()
    mp, acc = MatchParams(), np.zeros(8, dtype=np.uint32)
    lib().ppf_default_match_params(C.byref(mp))
    mp.presampled = 1
    pts = np.ascontiguousarray(bottle[:10], dtype=np.float32)
    fake_model = C.c_void_p(16)  # never dereferenced: the NULL workspace is refused first
    assert lib().ppf_debug_accumulators_ws(fake_model, None, pts.ctypes.data, 10, 6, 3, None, 0, 6, 3, C.byref(mp), acc.ctypes.data,
                                           acc.size, None) == _capi.PPF_ERR_INVALID
    assert "bad argument" in _capi.last_error()


def _write_model_file(path, n_ref=2, junk=b""):
    """A syntactically plausible header of the model file format (include/ppf_hip.h: ppf_model_save) followed by `junk`."""
    import struct
    tp = TrainParams()
    lib().ppf_default_train_params(C.byref(tp))
    info = _capi.ModelInfo()
    info.n_ref, info.num_angles, info.slots, info.n_buckets = n_ref, 30, 16, 1
    info.n_entries, info.n_tiles, info.tile_refs = n_ref * (n_ref - 1), 1, n_ref
    info.angle_step, info.distance_step, info.diameter = 2 * np.pi / 30, 0.01, 0.2
    with open(path, "wb") as f:
        f.write(b"PPFHIP05" + struct.pack("<II", 64, 0) + bytes(tp) + bytes(info) + struct.pack("<Q", 1) + junk)


def test_model_file_validation_is_host_side_and_loud(tmp_path):
    """ppf_model_check_file (the validation ppf_model_load runs before anything reaches a kernel) needs no device:
    missing, truncated, wrong-magic and inconsistent files are PPF_ERR_IO with a message, never an exception."""
    chk = lib().ppf_model_check_file
    assert chk(str(tmp_path / "nope.bin").encode()) == _capi.PPF_ERR_IO
    p = tmp_path / "m.bin"
    p.write_bytes(b"")
    assert chk(str(p).encode()) == _capi.PPF_ERR_IO
    p.write_bytes(b"NOTAMODEL" * 20)
    assert chk(str(p).encode()) == _capi.PPF_ERR_IO and "magic" in _capi.last_error()
    _write_model_file(p)  # header only: the tables are missing
    assert chk(str(p).encode()) == _capi.PPF_ERR_IO and "file size" in _capi.last_error()
    _write_model_file(p, n_ref=70000)  # N*N overflows the table's 31-bit pair index
    assert chk(str(p).encode()) == _capi.PPF_ERR_IO and "n_ref" in _capi.last_error()
    _write_model_file(p, junk=b"\xff" * 4096)  # right prefix, wrong size
    assert chk(str(p).encode()) == _capi.PPF_ERR_IO
    if lib().ppf_device_count() == 0:
        out = C.c_void_p()
        assert lib().ppf_model_load(str(p).encode(), C.byref(out)) == _capi.PPF_ERR_HIP


def test_block_cache_size_classes():
    """DevPool keying (host logic): a request is served from the smallest class that holds it, classes are 1/8 octave
    apart (at most 12.5 % waste above 2 KiB), and a block's own size maps back to its class, so a released block is found
    again by the next request of that size."""
    f = lib().ppf_debug_block_size
    assert f(0) == f(1) == f(256) == 256
    prev = 0
    rng = np.random.default_rng(0)
    sizes = sorted(set([257, 1000, 4096, 4097, 1 << 20, (1 << 20) + 1, 454_000_000, 4_269_982_720] +
                       [int(x) for x in rng.integers(300, 1 << 33, size=2000)]))
    for n in sizes:
        g = f(n)
        assert g >= n and f(g) == g, (n, g)
        if n >= 2048:
            assert g <= n * 1.125 + 1, (n, g)
        assert g >= prev
        prev = g
    assert len({f(n) for n in range(256, 4096)}) <= 8 * 4 + 1  # four octaves, eight classes each


def test_pool_guard_arguments_are_checked_before_the_device():
    """ppf_debug_pool_guard / ppf_debug_pool_check: a mode outside 0..2 and a NULL report are PPF_ERR_INVALID; without a device
    a valid call is PPF_ERR_HIP, as the compute entries are"""
    assert lib().ppf_debug_pool_guard(3) == _capi.PPF_ERR_INVALID and "mode" in _capi.last_error()
    assert lib().ppf_debug_pool_guard(-1) == _capi.PPF_ERR_INVALID
    assert lib().ppf_debug_pool_check(None) == _capi.PPF_ERR_INVALID
    if lib().ppf_device_count() == 0:
        r = _capi.PoolReport()
        assert lib().ppf_debug_pool_guard(1) == _capi.PPF_ERR_HIP and "no HIP device" in _capi.last_error()
        assert lib().ppf_debug_pool_check(C.byref(r)) == _capi.PPF_ERR_HIP


def test_workspace_options_are_checked_on_the_host():
    """ppf_workspace_create / _set_option / _destroy need no device: valid options are accepted, unknown ones and values out
    of range are PPF_ERR_INVALID with a message."""
    ws = C.c_void_p()
    assert lib().ppf_workspace_create(C.byref(ws)) == _capi.PPF_OK
    try:
        so = lib().ppf_workspace_set_option
        assert so(ws, _capi.PPF_OPT_HIT_FRACTION, C.c_double(0.1)) == _capi.PPF_OK
        assert so(ws, _capi.PPF_OPT_HIT_FRACTION, C.c_double(0.0)) == _capi.PPF_ERR_INVALID and "hit fraction" in _capi.last_error()
        assert so(ws, _capi.PPF_OPT_GROUP_ROUND_BUCKETS, C.c_double(1000)) == _capi.PPF_OK
        assert so(ws, _capi.PPF_OPT_CLUSTER_SERIAL, C.c_double(1)) == _capi.PPF_OK
        assert so(ws, _capi.PPF_OPT_ACC32, C.c_double(1)) == _capi.PPF_OK and so(ws, _capi.PPF_OPT_ACC32, C.c_double(0)) == _capi.PPF_OK
        assert so(ws, _capi.PPF_OPT_RUN_STAGING, C.c_double(64)) == _capi.PPF_OK and so(ws, _capi.PPF_OPT_RUN_STAGING, C.c_double(0)) == _capi.PPF_OK
        assert so(ws, _capi.PPF_OPT_RUN_STAGING, C.c_double(-1)) == _capi.PPF_ERR_INVALID and "run staging" in _capi.last_error()
        assert so(ws, 99, C.c_double(1)) == _capi.PPF_ERR_INVALID and "unknown option" in _capi.last_error()
        assert so(None, _capi.PPF_OPT_ACC32, C.c_double(1)) == _capi.PPF_ERR_INVALID
    finally:
        assert lib().ppf_workspace_destroy(ws) == _capi.PPF_OK
