"""The C-ABI surface of ppf_depth_volume_write and ppf_depth_volume_mesh without a GPU: the symbols are exported and bound, the
new records as a C and a C++ compiler lay them out equal their ctypes mirrors, the defaults, every argument error of _mesh,
_write, _info, _read and _release is PPF_ERR_INVALID before any device work, in the order the header states and with its
message, _write's per-record refusals name the record, and without a device a valid call is PPF_ERR_HIP.

Without a device the entries are handed a shell (ppf_debug_depth_volume_shell): a handle with the parameters and no device
memory.  With a device the volume is a real one, and a refused write must leave its bytes alone."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import DepthVolumeMeshParams, DepthVolumeMeshStats, DepthVolumeParams, VolumeMeshDesc, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_GPU = lib().ppf_device_count() > 0
ENTRIES = ["ppf_depth_volume_write", "ppf_default_depth_volume_mesh_params", "ppf_depth_volume_mesh", "ppf_volume_mesh_info",
           "ppf_volume_mesh_read", "ppf_volume_mesh_release"]
RECORDS = [
    ("ppf_depth_volume_mesh_params", DepthVolumeMeshParams, ["min_weight", "flags", "reserved"]),
    ("ppf_depth_volume_mesh_stats", DepthVolumeMeshStats, ["n_cells", "n_vertices", "n_triangles", "n_no_normal", "n_launches", "n_host_syncs",
                                                           "ms_wall", "reserved"]),
    ("ppf_volume_mesh_desc", VolumeMeshDesc, ["n_vertices", "n_triangles", "device_bytes", "reserved"]),
]
VOXEL = np.dtype([("d", "<f4"), ("w", "<i4")])
DIMS, MAX_WEIGHT = (8, 7, 6), 5
N = DIMS[0] * DIMS[1] * DIMS[2]
UNAVAILABLE = (_capi.PPF_ERR_INVALID, "shell") if HAVE_GPU else (_capi.PPF_ERR_HIP, "no HIP device")


def test_symbols_are_exported_and_bound():
    raw = C.CDLL(_capi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        res, args = _capi._SIGNATURES[name]
        assert list(getattr(lib(), name).argtypes) == list(args) and getattr(lib(), name).restype == res, name
    assert lib().ppf_abi_version() == _capi.PPF_ABI_VERSION == 4


def test_records_match_the_header(tmp_path):
    expr, got = [], []
    for cname, cls, fields in RECORDS:
        expr += [f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields]
        got += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
        assert [f for f, _ in cls._fields_] == fields and fields[-1] == "reserved" and C.sizeof(cls._fields_[-1][1]) == 16
    src = tmp_path / "vmsz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ppf_hip.h"\nint main(){\n' +
                   "".join(f'std::printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "vmsz"
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    assert got == [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    csrc = tmp_path / "vmsz.c"
    csrc.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppf_hip.h"\nint main(void){\n' +
                    "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    cexe = tmp_path / "vmszc"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(cexe)], check=True)
    assert got == [int(v) for v in subprocess.run([str(cexe)], check=True, capture_output=True, text=True).stdout.split()]


def mparams(**kw):
    p = DepthVolumeMeshParams()
    C.memset(C.byref(p), 0x09, C.sizeof(p))
    lib().ppf_default_depth_volume_mesh_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults():
    p = mparams()
    assert (p.min_weight, p.flags) == (1, 0) and list(p.reserved) == [0, 0, 0, 0]
    lib().ppf_default_depth_volume_mesh_params(None)   # no crash


def new_volume(entry):
    vp = DepthVolumeParams()
    lib().ppf_default_depth_volume_params(C.byref(vp))
    vp.dims[:], vp.origin[:] = DIMS, (-0.035, -0.03, 0.6)
    vp.voxel, vp.trunc, vp.max_weight = 0.01, 0.025, MAX_WEIGHT
    out = C.c_void_p()
    _capi.check(entry(C.byref(vp), C.byref(out)))
    return out


@pytest.fixture(scope="module")
def shell():
    out = new_volume(lib().ppf_debug_depth_volume_shell)
    yield out
    assert lib().ppf_depth_volume_release(out) == _capi.PPF_OK


@pytest.fixture(scope="module")
def volume():
    """a real volume with a device; without one the shell"""
    out = new_volume(lib().ppf_depth_volume_create if HAVE_GPU else lib().ppf_debug_depth_volume_shell)
    yield out
    assert lib().ppf_depth_volume_release(out) == _capi.PPF_OK


def records(**spoil):
    rec = np.empty(N, VOXEL)
    rec["d"], rec["w"] = np.linspace(-1.0, 1.0, N).astype(np.float32), np.arange(N) % (MAX_WEIGHT + 1)
    for index, (d, w) in spoil.items():
        rec[int(index[1:])] = (d, w)
    return rec


def mesh(v, mp=True, out=True, stats=True):
    o, st = C.c_void_p(0x5A5A), DepthVolumeMeshStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    prm = mparams() if mp is True else mp
    s = lib().ppf_depth_volume_mesh(v, C.byref(prm) if prm else None, C.byref(o) if out else None, C.byref(st) if stats else None)
    return s, o, st


def test_mesh_refuses_in_the_stated_order(shell):
    zero = bytes(C.sizeof(DepthVolumeMeshStats))
    # out NULL comes first, whatever else is wrong
    s, o, st = mesh(None, mp=None, out=False)
    assert s == _capi.PPF_ERR_INVALID and "ppf_depth_volume_mesh: out is NULL" in _capi.last_error() and bytes(st) == zero
    for what, v, mp, word in [("v and mp NULL", None, None, "the volume is NULL"), ("v NULL", None, True, "the volume is NULL"),
                              ("mp NULL", shell, None, "the mesh params are NULL"),
                              ("min_weight 0 and flags", shell, mparams(min_weight=0, flags=4), "min_weight must be >= 1"),
                              ("min_weight < 0", shell, mparams(min_weight=-3), "min_weight must be >= 1"),
                              ("flags", shell, mparams(flags=4), "unknown mesh flags 0x4")]:
        s, o, st = mesh(v, mp=mp)
        assert s == _capi.PPF_ERR_INVALID and word in _capi.last_error(), what
        assert o.value is None and bytes(st) == zero, what
    assert mesh(None, stats=False)[0] == _capi.PPF_ERR_INVALID   # stats may be NULL
    # past the checks: no device, or with one a shell that is no volume
    for mp in (True, mparams(min_weight=1 << 30)):
        s, o, st = mesh(shell, mp=mp)
        assert (s, UNAVAILABLE[1] in _capi.last_error()) == (UNAVAILABLE[0], True) and o.value is None and bytes(st) == zero


def test_write_refuses_in_the_stated_order(shell):
    write = lib().ppf_depth_volume_write
    rec = records()
    assert write(None, None, 0) == _capi.PPF_ERR_INVALID and "ppf_depth_volume_write: the volume is NULL" in _capi.last_error()
    assert write(shell, None, N + 1) == _capi.PPF_ERR_INVALID and "in is NULL" in _capi.last_error()
    for n in (0, N - 1, N + 1):
        bad = records(r0=(math.nan, 0))
        assert write(shell, bad.ctypes.data, n) == _capi.PPF_ERR_INVALID and f"in holds {n} records, the volume has {N} voxels" in _capi.last_error()
    assert write(shell, rec.ctypes.data, N) == UNAVAILABLE[0] and UNAVAILABLE[1] in _capi.last_error()


RECORD_INVALID = [("w < 0", 17, (0.25, -1)), ("w above max_weight", 0, (0.25, MAX_WEIGHT + 1)), ("d nan", N - 1, (math.nan, 1)),
                  ("d inf", 5, (math.inf, 1)), ("d -inf", 6, (-math.inf, 0)), ("d above 1", 100, (float(np.nextafter(np.float32(1), np.float32(2))), 1)),
                  ("d below -1", 101, (float(np.nextafter(np.float32(-1), np.float32(-2))), 2))]


@pytest.mark.parametrize("what,index,record", RECORD_INVALID, ids=[r[0] for r in RECORD_INVALID])
def test_write_refuses_a_record_and_names_it(volume, what, index, record):
    write = lib().ppf_depth_volume_write
    before = np.empty(N, VOXEL)
    if HAVE_GPU:
        _capi.check(lib().ppf_depth_volume_read(volume, before.ctypes.data, N))
    # the first bad record fails the call: a later one is not the one named
    rec = records(**{f"r{index}": record, f"r{N - 1}": (math.nan, -7)} if index != N - 1 else {f"r{index}": record})
    assert write(volume, rec.ctypes.data, N) == _capi.PPF_ERR_INVALID
    msg = _capi.last_error()
    assert f"ppf_depth_volume_write: record {index} has" in msg and f"0..{MAX_WEIGHT}" in msg and "[-1, 1]" in msg, msg
    if HAVE_GPU:
        after = np.empty(N, VOXEL)
        _capi.check(lib().ppf_depth_volume_read(volume, after.ctypes.data, N))
        assert before.tobytes() == after.tobytes()


def test_write_accepts_the_ends_of_every_range(shell):
    rec = records(r3=(1.0, MAX_WEIGHT), r4=(-1.0, 0), r5=(-0.0, 0))
    assert lib().ppf_depth_volume_write(shell, rec.ctypes.data, N) == UNAVAILABLE[0] and UNAVAILABLE[1] in _capi.last_error()


def test_info_read_and_release_check_their_arguments():
    d = VolumeMeshDesc()
    C.memset(C.byref(d), 0x5A, C.sizeof(d))
    assert lib().ppf_volume_mesh_info(None, C.byref(d)) == _capi.PPF_ERR_INVALID and "ppf_volume_mesh_info" in _capi.last_error()
    assert bytes(d) == bytes(C.sizeof(d))
    assert lib().ppf_volume_mesh_info(None, None) == _capi.PPF_ERR_INVALID
    v, t = np.full(6, 7.0, np.float32), np.full(3, 7, np.int32)
    assert lib().ppf_volume_mesh_read(None, v.ctypes.data, 1, t.ctypes.data, 1) == _capi.PPF_ERR_INVALID
    assert "ppf_volume_mesh_read: the mesh is NULL" in _capi.last_error() and (v == 7.0).all() and (t == 7).all()
    assert lib().ppf_volume_mesh_read(None, None, 0, None, 0) == _capi.PPF_ERR_INVALID
    assert lib().ppf_volume_mesh_release(None) == _capi.PPF_OK


def test_python_wrappers_without_a_device():
    from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DepthVolume, VolumeMesh
    assert callable(DepthVolume.write) and callable(DepthVolume.mesh) and callable(VolumeMesh.save_ply)
    cp = CloudProcessor(None, np.zeros((4, 4), np.float32), [], [], [], 0.05, 0.05)
    with pytest.raises(_capi.PPFError) as e:
        cp.MeshVolume()
    assert e.value.status == _capi.PPF_ERR_INVALID and "FuseVolume" in str(e.value)


FACADE_PROGRAM = r"""
#include <cstdio>
#include <iostream>
#include "ppf_cloud_stages.hpp"
using namespace ppfhip;
int main() {
  try {
    ppf_depth_volume_params vp = prep::DepthVolume::defaultParams();
    vp.dims[0] = vp.dims[1] = vp.dims[2] = 4;
    vp.voxel = 0.01f; vp.trunc = 0.025f; vp.origin[0] = vp.origin[1] = -0.015; vp.origin[2] = 0.6;
    prep::DepthVolume volume(vp);
    std::vector<ppf_depth_volume_voxel> rec(64);
    for (int q = 0; q < 64; q++) { rec[q].d = (q / 16) < 2 ? 0.5f : -0.5f; rec[q].w = 1; }   /* a plane between k = 1 and k = 2 */
    volume.write(rec);
    ppf_depth_volume_mesh_stats st;
    const prep::VolumeMesh m = volume.mesh(1, &st);
    std::printf("%d %d %lld %lld %lld\n", m.nVertices(), m.nTriangles(), (long long)st.n_cells, (long long)st.n_no_normal,
                (long long)volume.read().size());
  } catch (const ppf_match_3d::Error& e) {
    std::cerr << e.what() << std::endl;
    return 10 + e.status;
  }
  return 0;
}
"""


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_the_cxx_facade_compiles_as_cxx11_and_runs(tmp_path, compiler):
    """prep::DepthVolume::write and ::mesh, warnings as errors; without a device the program ends with PPF_ERR_HIP's exit code,
    with one its counts are the oracle's"""
    csrc = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
    src = tmp_path / "mesh_facade.cpp"
    src.write_text(FACADE_PROGRAM)
    exe = str(tmp_path / "mesh_facade")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", csrc,
                    "-lppf_hip", f"-Wl,-rpath,{csrc}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    if not HAVE_GPU:
        assert r.returncode == 10 + _capi.PPF_ERR_HIP and "no HIP device" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    import depth_volume_oracle as O
    import volume_mesh_oracle as M
    ov = O.Volume((4, 4, 4), 0.01, (-0.015, -0.015, 0.6), trunc=0.025)
    ov.d[...] = np.where(np.arange(4)[:, None, None] < 2, np.float32(0.5), np.float32(-0.5))
    ov.w[...] = 1
    v, t, st = M.mesh(ov, 1)
    assert [int(x) for x in r.stdout.split()] == [len(v), len(t), st["n_cells"], st["n_no_normal"], 64] and len(t) > 0


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_the_demo_is_cxx11(tmp_path, compiler):
    """examples/volume_mesh_demo.cpp and the facade behind it, warnings as errors; a file it cannot read is its own exit code"""
    csrc = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
    exe = str(tmp_path / "volume_mesh_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "volume_mesh_demo.cpp"), "-L", csrc, "-lppf_hip", f"-Wl,-rpath,{csrc}", "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True).returncode == 1
    r = subprocess.run([exe, str(tmp_path / "missing.f32"), str(tmp_path / "missing.f64"), "2", "4", "4", "1", "1", "0", "0", "8", "8", "8", "0.01",
                        "0", "0", "0.5", "0.03", "0.004"], capture_output=True, text=True)
    assert r.returncode == 10 + _capi.PPF_ERR_IO and "cannot read" in r.stderr
