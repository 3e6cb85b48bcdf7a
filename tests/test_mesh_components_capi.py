"""The C-ABI surface of ppf_volume_mesh_upload and ppf_volume_mesh_components without a GPU: the symbols are exported and bound,
the three records as a C and a C++ compiler lay them out equal their ctypes mirrors, the defaults, every argument error of
both entries is PPF_ERR_INVALID before any device work, in the order the header states, with its message and the index it
names; *out and *stats after a failure; and without a device a valid call is PPF_ERR_HIP.

Without a device _components is handed a shell (ppf_debug_volume_mesh_shell): a handle with the counts and no device memory."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import MeshComponentInfo, MeshComponentParams, MeshComponentStats, lib

import mesh_components_oracle as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_GPU = lib().ppf_device_count() > 0
INT32_MAX = 2 ** 31 - 1
ENTRIES = ["ppf_volume_mesh_upload", "ppf_default_mesh_component_params", "ppf_volume_mesh_components", "ppf_debug_volume_mesh_shell"]
RECORDS = [
    ("ppf_mesh_component_params", MeshComponentParams, ["min_triangles", "min_area", "rank_lo", "rank_hi", "flags", "reserved"]),
    ("ppf_mesh_component_info", MeshComponentInfo, ["n_vertices", "n_triangles", "n_degenerate", "n_edges", "n_boundary_edges",
                                                    "n_nonmanifold_edges", "first_vertex", "kept", "area", "lo", "hi", "reserved"]),
    ("ppf_mesh_component_stats", MeshComponentStats, ["n_components", "n_kept", "n_unreferenced", "n_bad_area", "n_vertices_out",
                                                      "n_triangles_out", "n_launches", "n_host_syncs", "ms_wall", "reserved"]),
]
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
        assert [f for f, _ in cls._fields_] == fields and fields[-1] == "reserved"
    assert [C.sizeof(cls) for _, cls, _ in RECORDS] == [32, 72, 80]
    # the oracle's numpy record is the C record
    assert MC.INFO.itemsize == C.sizeof(MeshComponentInfo)
    assert [MC.INFO.fields[f][1] for f in RECORDS[1][2]] == [getattr(MeshComponentInfo, f).offset for f in RECORDS[1][2]]
    for ext, std, cc, head in (("cpp", "-std=c++11", "g++", "#include <cstdio>\n#include <cstddef>\n"),
                               ("c", "-std=c99", "gcc", "#include <stdio.h>\n#include <stddef.h>\n")):
        src = tmp_path / f"mcsz.{ext}"
        src.write_text(head + '#include "ppf_hip.h"\nint main(void){\n' + "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
        exe = tmp_path / f"mcsz_{ext}"
        subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        assert got == [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()], cc


def cparams(**kw):
    p = MeshComponentParams()
    C.memset(C.byref(p), 0x09, C.sizeof(p))
    lib().ppf_default_mesh_component_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults():
    p = cparams()
    assert (p.min_triangles, p.min_area, p.rank_lo, p.rank_hi, p.flags) == (1, 0.0, 0, INT32_MAX, 0) and list(p.reserved) == [0, 0, 0]
    lib().ppf_default_mesh_component_params(None)   # no crash


# ---- upload ----------------------------------------------------------------------------------------------------------
V = np.arange(5 * 8, dtype=np.float32).reshape(5, 8)
T = np.array([[0, 1, 2], [2, 3, 4], [4, 0, 1]], np.int32)


def upload(v=V, nv=5, stride=8, noff=5, t=T, nt=3, out=True):
    o = C.c_void_p(0x5A5A)
    s = lib().ppf_volume_mesh_upload(v.ctypes.data if v is not None else None, nv, stride, noff, t.ctypes.data if t is not None else None, nt,
                                     C.byref(o) if out else None)
    return s, o


def spoiled(a, index, value):
    b = a.copy()
    b[index] = value
    return b


UPLOAD_INVALID = [
    ("n_vertices < 0", dict(nv=-1, stride=2, t=None), "n_vertices is -1"),
    ("n_vertices above INT32_MAX", dict(nv=INT32_MAX + 1, nt=-4), f"n_vertices is {INT32_MAX + 1}"),
    ("n_triangles < 0", dict(nt=-4, v=None), "n_triangles is -4"),
    ("n_triangles above INT32_MAX", dict(nt=INT32_MAX + 1, v=None), f"n_triangles is {INT32_MAX + 1}"),
    ("vertices NULL", dict(v=None, t=None, stride=1), "vertices is NULL"),
    ("triangles NULL", dict(t=None, stride=1), "triangles is NULL"),
    ("vstride 2", dict(stride=2, noff=7), "vstride is 2"),
    ("offset -2", dict(noff=-2, v=spoiled(V, (0, 0), math.nan)), "normal_offset -2 does not fit a row of 8 floats"),
    ("offset past the row", dict(noff=6), "normal_offset 6 does not fit a row of 8 floats"),
    ("x nan", dict(v=spoiled(spoiled(V, (3, 0), math.nan), (4, 1), math.inf), t=spoiled(T, (0, 0), 9)), "vertex 3 has a position"),
    ("y inf", dict(v=spoiled(V, (0, 1), math.inf)), "vertex 0 has a position"),
    ("z -inf", dict(v=spoiled(V, (4, 2), -math.inf)), "vertex 4 has a position"),
    ("index 5", dict(t=spoiled(spoiled(T, (1, 2), 5), (2, 0), -1)), "triangle 1 names vertex 5 of 5"),
    ("index -1", dict(t=spoiled(T, (2, 0), -1)), "triangle 2 names vertex -1 of 5"),
    ("index with fewer vertices", dict(nv=4), "triangle 1 names vertex 4 of 4"),
]


@pytest.mark.parametrize("what,kw,word", UPLOAD_INVALID, ids=[u[0] for u in UPLOAD_INVALID])
def test_upload_refuses_in_the_stated_order(what, kw, word):
    s, o = upload(**kw)
    assert s == _capi.PPF_ERR_INVALID and "ppf_volume_mesh_upload: " + word in _capi.last_error(), _capi.last_error()
    assert o.value is None


def test_upload_out_null_comes_first_and_a_valid_call_needs_a_device():
    s, _ = upload(nv=-1, out=False)
    assert s == _capi.PPF_ERR_INVALID and "ppf_volume_mesh_upload: out is NULL" in _capi.last_error()
    # a normal is not a position: it may hold anything
    for kw in (dict(), dict(noff=-1), dict(stride=3, noff=-1, v=np.ascontiguousarray(V[:, :3])), dict(v=spoiled(V, (2, 6), math.nan)),
               dict(v=None, nv=0, t=None, nt=0)):
        s, o = upload(**kw)
        if HAVE_GPU:
            assert s == _capi.PPF_OK and o.value and lib().ppf_volume_mesh_release(o) == _capi.PPF_OK
        else:
            assert s == _capi.PPF_ERR_HIP and "ppf_volume_mesh_upload: no HIP device" in _capi.last_error() and o.value is None


# ---- components ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shell():
    out = C.c_void_p()
    _capi.check(lib().ppf_debug_volume_mesh_shell(5, 3, C.byref(out)))
    d = _capi.VolumeMeshDesc()
    _capi.check(lib().ppf_volume_mesh_info(out, C.byref(d)))
    assert (d.n_vertices, d.n_triangles, d.device_bytes) == (5, 3, 0)
    yield out
    assert lib().ppf_volume_mesh_release(out) == _capi.PPF_OK


def components(m, p=True, out=True, stats=True, info=True, cap=4):
    o, st = C.c_void_p(0x5A5A), MeshComponentStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    prm = cparams() if p is True else p
    rec = (MeshComponentInfo * 4)()
    lab = np.full(5, -7, np.int32)
    s = lib().ppf_volume_mesh_components(m, C.byref(prm) if prm else None, C.byref(o) if out else None, lab.ctypes.data, rec if info else None, cap,
                                         C.byref(st) if stats else None)
    assert (lab == -7).all() and bytes(rec) == bytes(C.sizeof(rec))
    return s, o, st


def test_components_refuses_in_the_stated_order(shell):
    zero = bytes(C.sizeof(MeshComponentStats))
    nan, inf = math.nan, math.inf
    for what, m, p, kw, word in [
            ("m and p NULL", None, None, {}, "the mesh is NULL"),
            ("m NULL", None, True, {}, "the mesh is NULL"),
            ("p NULL", shell, None, dict(cap=-1), "the component params are NULL"),
            ("min_triangles 0", shell, cparams(min_triangles=0, min_area=-1.0), {}, "min_triangles must be >= 1"),
            ("min_triangles < 0", shell, cparams(min_triangles=-5), {}, "min_triangles must be >= 1"),
            ("min_area < 0", shell, cparams(min_area=-1e-9, rank_lo=-1), {}, "min_area must be finite and >= 0"),
            ("min_area nan", shell, cparams(min_area=nan), {}, "min_area must be finite and >= 0"),
            ("min_area inf", shell, cparams(min_area=inf), {}, "min_area must be finite and >= 0"),
            ("rank_lo < 0", shell, cparams(rank_lo=-1, rank_hi=-2), {}, "rank_lo must be >= 0"),
            ("rank_hi < rank_lo", shell, cparams(rank_lo=3, rank_hi=2, flags=1), {}, "rank_hi must be >= rank_lo"),
            ("flags", shell, cparams(flags=4), dict(cap=-1), "unknown component flags 0x4"),
            ("cap_info < 0", shell, True, dict(cap=-1, info=False), "cap_info is -1"),
            ("info NULL", shell, True, dict(cap=2, info=False), "info is NULL with cap_info 2")]:
        for out in (True, False):
            s, o, st = components(m, p=p, out=out, **kw)
            assert s == _capi.PPF_ERR_INVALID and "ppf_volume_mesh_components: " + word in _capi.last_error(), (what, _capi.last_error())
            assert bytes(st) == zero and (o.value is None if out else o.value == 0x5A5A), what
    assert components(None, stats=False)[0] == _capi.PPF_ERR_INVALID   # stats may be NULL
    # past the checks: no device, or with one a shell that is no mesh
    for p, kw in ((True, {}), (cparams(rank_lo=2, rank_hi=2, min_area=0.0, min_triangles=INT32_MAX), dict(cap=0, info=False)), (True, dict(out=False))):
        s, o, st = components(shell, p=p, **kw)
        assert (s, UNAVAILABLE[1] in _capi.last_error()) == (UNAVAILABLE[0], True) and bytes(st) == zero
        assert o.value is None or not kw.get("out", True)


def test_the_shell_checks_its_arguments():
    out = C.c_void_p(0x5A5A)
    assert lib().ppf_debug_volume_mesh_shell(1, 1, None) == _capi.PPF_ERR_INVALID
    assert lib().ppf_debug_volume_mesh_shell(-1, 1, C.byref(out)) == _capi.PPF_ERR_INVALID and out.value is None


def test_python_wrappers_without_a_device():
    from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, VolumeMesh
    assert all(callable(getattr(VolumeMesh, n)) for n in ("from_arrays", "components", "largest", "split"))
    cp = CloudProcessor(None, np.zeros((4, 4), np.float32), [], [], [], 0.05, 0.05)
    for call in (lambda: cp.MeshVolume(keep_largest=1), lambda: cp.MeshVolumeObjects(2, min_triangles=100)):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID and "FuseVolume" in str(e.value)
    with pytest.raises(_capi.PPFError) as e:
        VolumeMesh.from_arrays(np.zeros((3, 4), np.float32), np.zeros((1, 3), np.int32))
    assert e.value.status == _capi.PPF_ERR_INVALID
    if not HAVE_GPU:
        with pytest.raises(_capi.PPFError) as e:
            VolumeMesh.from_arrays(*MC.hand_made()["tetrahedron"])
        assert e.value.status == _capi.PPF_ERR_HIP


FACADE_PROGRAM = r"""
#include <cstdio>
#include <iostream>
#include "ppf_cloud_stages.hpp"
using namespace ppfhip;
int main() {
  try {
    /* two triangles that share nothing, the second larger, and a vertex that nothing names */
    const float v[7 * 3] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 9, 9, 9, 5, 0, 0, 7, 0, 0, 5, 2, 0};
    const int32_t t[2 * 3] = {0, 1, 2, 4, 5, 6};
    const prep::VolumeMesh m = prep::VolumeMesh::fromArrays(v, 7, 3, -1, t, 2);
    std::vector<ppf_mesh_component_info> info;
    std::vector<int32_t> labels;
    ppf_mesh_component_stats st;
    const prep::VolumeMesh all = m.components(0, &info, 8, &labels, &st);
    const prep::VolumeMesh big = m.largest(1);
    std::printf("%d %d %d %d %lld %lld %d %d %d %d %d %g %d %d\n", m.nVertices(), m.nTriangles(), all.nVertices(), all.nTriangles(),
                (long long)st.n_components, (long long)st.n_unreferenced, (int)info.size(), info[0].first_vertex, labels[0], labels[3], labels[4],
                info[0].area, big.nVertices(), big.triangles[2]);
  } catch (const ppf_match_3d::Error& e) {
    std::cerr << e.what() << std::endl;
    return 10 + e.status;
  }
  return 0;
}
"""


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_the_cxx_facade_compiles_as_cxx11_and_runs(tmp_path, compiler):
    """prep::VolumeMesh::fromArrays, ::components and ::largest, warnings as errors; without a device the program ends with
    PPF_ERR_HIP's exit code, with one its figures are the known ones"""
    csrc = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
    src = tmp_path / "components_facade.cpp"
    src.write_text(FACADE_PROGRAM)
    exe = str(tmp_path / "components_facade")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L", csrc,
                    "-lppf_hip", f"-Wl,-rpath,{csrc}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    if not HAVE_GPU:
        assert r.returncode == 10 + _capi.PPF_ERR_HIP and "no HIP device" in r.stderr
        return
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["7", "2", "6", "2", "2", "1", "2", "4", "1", "-1", "0", "2", "3", "2"]


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_the_demo_is_cxx11(tmp_path, compiler):
    """examples/mesh_components_demo.cpp and the facade behind it, warnings as errors; a file it cannot read is its own exit code"""
    csrc = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
    exe = str(tmp_path / "mesh_components_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "mesh_components_demo.cpp"), "-L", csrc, "-lppf_hip", f"-Wl,-rpath,{csrc}", "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True).returncode == 1
    r = subprocess.run([exe, str(tmp_path / "missing.f32"), str(tmp_path / "missing.f64"), "2", "4", "4", "1", "1", "0", "0", "8", "8", "8", "0.01",
                        "0", "0", "0.5", "0.03", "100"], capture_output=True, text=True)
    assert r.returncode == 10 + _capi.PPF_ERR_IO and "cannot read" in r.stderr
