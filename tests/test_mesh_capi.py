"""ppf_cloud_from_mesh without a device: the symbols, the two records against the header under g++ and gcc, the defaults, every
argument error with its message and the zeroed outputs in the header's order, the host's capacity count, PPF_ERR_HIP, the PLY
mesh reader and writer, and the C++ facade and demo as C++11."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import mesh_cases as MC
import mesh_oracle as MO
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import MeshSampleParams, MeshSampleStats, lib
from yolo_ppf_pose_estimation_amd.ply import load_ply_mesh, load_ply_simple, write_ply, write_ply_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_GPU = lib().ppf_device_count() > 0
ENTRIES = ["ppf_default_mesh_sample_params", "ppf_cloud_from_mesh"]
RECORDS = [("ppf_mesh_sample_params", MeshSampleParams,
            ["spacing", "seed", "normals", "visibility", "map_size", "min_views", "depth_tol", "orient", "max_rows", "reserved"]),
           ("ppf_mesh_sample_stats", MeshSampleStats,
            ["n_triangles", "n_degenerate", "n_sampled", "n_hidden", "n_flipped", "n_rows", "n_large", "n_launches", "n_host_syncs",
             "area", "reserved"])]


def test_symbols_are_exported_and_bound():
    raw = C.CDLL(_capi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        res, args = _capi._SIGNATURES[name]
        assert list(getattr(lib(), name).argtypes) == list(args) and getattr(lib(), name).restype == res, name


def test_records_match_the_header(tmp_path):
    consts = ["PPF_MESH_NORMALS_FACE", "PPF_MESH_NORMALS_VERTEX", "PPF_MESH_VIEWS", "PPF_MESH_HOST_COUNT", "PPF_ABI_VERSION"]
    expr, got = [], []
    for cname, cls, fields in RECORDS:
        expr += [f"sizeof({cname})"] + [f"offsetof({cname}, {f})" for f in fields]
        got += [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
        assert [f for f, _ in cls._fields_] == fields and fields[-1] == "reserved" and C.sizeof(cls._fields_[-1][1]) == 16
    expr += consts
    got += [getattr(_capi, c) for c in consts]
    src = tmp_path / "msz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ppf_hip.h"\nint main(){\n' +
                   "".join(f'std::printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "msz"
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert want[-5:] == [0, 1, 26, 1024, 4]   # the interface only grows: the ABI version stays
    csrc = tmp_path / "msz.c"
    csrc.write_text('#include <stdio.h>\n#include "ppf_hip.h"\nint main(void){printf("' + "%zu " * len(RECORDS) + '\\n", ' +
                    ", ".join(f"sizeof({c})" for c, _, _ in RECORDS) + ");return 0;}\n")
    cexe = tmp_path / "mszc"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(csrc), "-o", str(cexe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(cexe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [C.sizeof(cls) for _, cls, _ in RECORDS] == [52, 88]


def params(**kw):
    p = MeshSampleParams()
    C.memset(C.byref(p), 0x09, C.sizeof(p))
    lib().ppf_default_mesh_sample_params(C.byref(p))
    for k, v in kw.items():
        if k == "reserved":
            p.reserved[:] = v
        else:
            setattr(p, k, v)
    return p


def test_defaults():
    p = params()
    assert p.spacing == float(np.float32(0.004)) and p.seed == 0 and p.normals == _capi.PPF_MESH_NORMALS_FACE
    assert (p.visibility, p.map_size, p.min_views, p.depth_tol, p.orient, p.max_rows) == (1, 0, 0, 0.0, 1, 0)
    assert list(p.reserved) == [0, 0, 0, 0]
    lib().ppf_default_mesh_sample_params(None)   # tolerated


V8, T12 = MC.box()


def call(V=V8, T=T12, n_vertices=None, vstride=None, normal_offset=-1, n_triangles=None, p=None, out="fresh", null_vertices=False,
         null_triangles=False, null_params=False):
    """the raw entry with spoiled outputs: (status, message, out handle value, stats bytes)"""
    V = np.ascontiguousarray(V, dtype=np.float32)
    T = np.ascontiguousarray(T, dtype=np.int32)
    st = MeshSampleStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    handle = C.c_void_p(0xDEAD)
    p = params() if p is None else p
    s = lib().ppf_cloud_from_mesh(None if null_vertices else V.ctypes.data, len(V) if n_vertices is None else n_vertices,
                                  V.shape[1] if vstride is None else vstride, normal_offset, None if null_triangles else T.ctypes.data,
                                  len(T) if n_triangles is None else n_triangles, None if null_params else C.byref(p),
                                  None if out is None else C.byref(handle), C.byref(st))
    return s, _capi.last_error(), handle.value, bytes(st)


ZERO = bytes(C.sizeof(MeshSampleStats))
V6 = np.concatenate([V8, V8], axis=1)

REFUSALS = [
    ("params NULL", dict(null_params=True), "params are NULL"),
    ("vertices NULL", dict(null_vertices=True), "must not be NULL"),
    ("triangles NULL", dict(null_triangles=True), "must not be NULL"),
    ("no vertices", dict(n_vertices=0), "0 vertices"),
    ("no triangles", dict(n_triangles=0), "0 triangles"),
    ("negative triangles", dict(n_triangles=-1), "-1 triangles"),
    ("vstride 2", dict(vstride=2), "vstride 2"),
    ("normal_offset 2", dict(V=V6, normal_offset=2), "normal_offset 2"),
    ("normal_offset -2", dict(V=V6, normal_offset=-2), "normal_offset -2"),
    ("normal_offset past the stride", dict(V=V6, normal_offset=4), "normal_offset 4"),
    ("normal_offset with vstride 3", dict(normal_offset=3), "normal_offset 3"),
    ("spacing 0", dict(p=params(spacing=0.0)), "spacing"),
    ("spacing negative", dict(p=params(spacing=-0.004)), "spacing"),
    ("spacing NaN", dict(p=params(spacing=float("nan"))), "spacing"),
    ("spacing inf", dict(p=params(spacing=float("inf"))), "spacing"),
    ("normals 2", dict(p=params(normals=2)), "normals 2"),
    ("normals -1", dict(p=params(normals=-1)), "normals -1"),
    ("vertex normals without an offset", dict(p=params(normals=1)), "needs a normal_offset"),
    ("visibility 2", dict(p=params(visibility=2)), "visibility 2"),
    ("orient 2", dict(p=params(orient=2)), "orient 2"),
    ("orient without visibility", dict(p=params(visibility=0)), "orient needs visibility"),
    ("map_size 15", dict(p=params(map_size=15)), "map_size 15"),
    ("map_size 1025", dict(p=params(map_size=1025)), "map_size 1025"),
    ("map_size -1", dict(p=params(map_size=-1)), "map_size -1"),
    ("min_views -1", dict(p=params(min_views=-1)), "min_views -1"),
    ("min_views 27", dict(p=params(min_views=27)), "min_views 27"),
    ("depth_tol negative", dict(p=params(depth_tol=-0.001)), "depth_tol"),
    ("depth_tol NaN", dict(p=params(depth_tol=float("nan"))), "depth_tol"),
    ("max_rows negative", dict(p=params(max_rows=-1)), "max_rows -1"),
    ("reserved", dict(p=params(reserved=[0, 0, 1, 0])), "reserved"),
    ("index 8", dict(T=np.array([[0, 1, 2], [0, 8, 1]])), "triangle 1 has index 8"),
    ("index -1", dict(T=np.array([[0, -1, 2]])), "triangle 0 has index -1"),
]


@pytest.mark.parametrize("what,kw,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_any_device_work(what, kw, word):
    s, msg, handle, st = call(**kw)
    assert s == _capi.PPF_ERR_INVALID and msg.startswith("ppf_cloud_from_mesh: ") and word in msg, msg
    assert handle is None and st == ZERO


def test_out_null_and_the_order_of_the_checks():
    s, msg, _, st = call(out=None, null_params=True)
    assert s == _capi.PPF_ERR_INVALID and "out is NULL" in msg and st == ZERO
    # each refusal wins over every later one
    order = [(dict(null_params=True), "params are NULL"), (dict(null_vertices=True), "must not be NULL"), (dict(n_vertices=0), "0 vertices"),
             (dict(vstride=2), "vstride"), (dict(normal_offset=7), "normal_offset"), (dict(p=dict(spacing=0.0)), "spacing"),
             (dict(p=dict(normals=5)), "normals 5"), (dict(p=dict(visibility=3)), "visibility"), (dict(p=dict(orient=-1)), "orient -1"),
             (dict(p=dict(map_size=8)), "map_size"), (dict(p=dict(min_views=99)), "min_views"), (dict(p=dict(depth_tol=-1.0)), "depth_tol"),
             (dict(p=dict(max_rows=-5)), "max_rows"), (dict(p=dict(reserved=[1, 0, 0, 0])), "reserved"),
             (dict(T=np.array([[0, 1, 99]])), "index 99")]
    for i, (_, word) in enumerate(order):
        kw, pk = {}, {}
        for later, _ in order[i:]:
            for k, v in later.items():
                if k == "p":
                    pk.update(v)
                else:
                    kw.setdefault(k, v)
        if pk:
            kw["p"] = params(**pk)
        s, msg, handle, st = call(**kw)
        assert s == _capi.PPF_ERR_INVALID and word in msg, (i, word, msg)
        assert handle is None and st == ZERO
    # vertex normals without an offset, orient without visibility: behind the field's own range check
    assert "needs a normal_offset" in call(p=params(normals=1, visibility=2))[1]
    assert "visibility 2" in call(p=params(orient=2, visibility=2))[1]
    assert "orient needs visibility" in call(p=params(visibility=0, map_size=1))[1]


def test_a_small_mesh_is_counted_on_the_host():
    """the box at 4 mm gives 7,749 or so rows: max_rows below that is PPF_ERR_CAPACITY without a device, by the sum or by one
    triangle's q alone; the host's count is the oracle's"""
    n = MO.mesh_sample(V8, T12, 0.004, visibility=0, orient=0)["stats"]["n_sampled"]
    assert 7700 < n < 7800
    for cap in (n - 1, 800, 1):
        s, msg, handle, st = call(p=params(max_rows=cap))
        assert s == _capi.PPF_ERR_CAPACITY and f"max_rows = {cap} rows" in msg and handle is None and st == ZERO
    for cap in (n, 0):   # exactly max_rows is allowed, and the default is 2^24: the call gets as far as the device question
        s, msg, handle, st = call(p=params(max_rows=cap))
        assert (s == _capi.PPF_OK) if HAVE_GPU else (s == _capi.PPF_ERR_HIP and "no HIP device" in msg and handle is None and st == ZERO)
        if s == _capi.PPF_OK:
            lib().ppf_cloud_release(C.c_void_p(handle))
    with pytest.raises(MO.MeshCapacity):
        MO.mesh_sample(V8, T12, 0.004, max_rows=n - 1)
    # a degenerate triangle in the list is skipped, an all-degenerate list counts nothing
    Vd, Td = MC.all_degenerate()
    s = call(V=Vd, T=Td, p=params(max_rows=1))[0]
    assert s == (_capi.PPF_OK if HAVE_GPU else _capi.PPF_ERR_HIP)


def test_valid_arguments_reach_the_device_question():
    if HAVE_GPU:
        pytest.skip("a GPU is present")
    Vt, Tt = MC.torus(with_normals=True, vstride=8, normal_offset=4)
    for kw in (dict(), dict(V=Vt, T=Tt, normal_offset=4, p=params(normals=1, map_size=16, min_views=26)),
               dict(V=Vt, T=Tt, normal_offset=5, p=params(visibility=0, orient=0, map_size=1024, min_views=1, depth_tol=0.5))):
        s, msg, handle, st = call(**kw)
        assert s == _capi.PPF_ERR_HIP and "no HIP device" in msg and handle is None and st == ZERO
    from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud
    with pytest.raises(_capi.PPFError) as e:
        DeviceCloud.from_mesh(V8, T12, 0.004)
    assert e.value.status == _capi.PPF_ERR_HIP
    with pytest.raises(_capi.PPFError) as e:
        CloudProcessor().LoadMeshModel((V8, T12), "box")
    assert e.value.status == _capi.PPF_ERR_HIP


def test_python_wrappers_check_their_arguments():
    from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud
    for bad in (dict(vertices=V8.reshape(-1), triangles=T12), dict(vertices=V8, triangles=T12[:, :2]), dict(vertices=V8, triangles=T12, normals="smooth")):
        kw = dict(bad)
        with pytest.raises(_capi.PPFError) as e:
            DeviceCloud.from_mesh(kw.pop("vertices"), kw.pop("triangles"), 0.004, **kw)
        assert e.value.status == _capi.PPF_ERR_INVALID and "from_mesh" in str(e.value)
    with pytest.raises(_capi.PPFError) as e:
        DeviceCloud.from_mesh(V8, T12, 0.004, normals="vertex")
    assert e.value.status == _capi.PPF_ERR_INVALID and "needs a normal_offset" in str(e.value)
    with pytest.raises(_capi.PPFError) as e:
        DeviceCloud.from_mesh(V8, T12, -1.0)
    assert "spacing" in str(e.value)


# ---- PLY meshes ------------------------------------------------------------------------------------------------------------
def test_ply_mesh_round_trip_ascii(tmp_path):
    for V, T in (MC.box(), MC.torus(nu=6, nv=4, with_normals=True)):
        path = str(tmp_path / "m.ply")
        write_ply_mesh(V, T, path)
        V2, T2 = load_ply_mesh(path)
        assert V2.dtype == np.float32 and T2.dtype == np.int32 and V2.tobytes() == V.tobytes() and T2.tobytes() == T.tobytes()
        rows = load_ply_simple(path, with_normals=V.shape[1] >= 6)    # the vertex list reader still reads the written file
        assert rows.shape == V.shape and rows[:, :3].tobytes() == V[:, :3].tobytes()


def _binary_ply(path, V, faces, extra=True, index_name="vertex_index"):
    """binary_little_endian with a comment, an extra vertex property between z and nx, an extra face property and an element after"""
    with open(path, "wb") as fh:
        head = ["ply", "format binary_little_endian 1.0", "comment made by a test", f"element vertex {len(V)}",
                "property float x", "property float y", "property float z"]
        head += ["property uchar quality"] if extra else []
        head += ["property float nx", "property float ny", "property float nz"] if V.shape[1] >= 6 else []
        head += [f"element face {len(faces)}", f"property list uchar int {index_name}"] + (["property short flags"] if extra else [])
        head += ["element edge 1", "property int vertex1", "property int vertex2", "end_header"]
        fh.write(("\n".join(head) + "\n").encode())
        for v in V:
            fh.write(struct.pack("<3f", *v[:3]))
            if extra:
                fh.write(struct.pack("<B", 200))
            if V.shape[1] >= 6:
                fh.write(struct.pack("<3f", *v[3:6]))
        for f in faces:
            fh.write(struct.pack(f"<B{len(f)}i", len(f), *f))
            if extra:
                fh.write(struct.pack("<h", -3))
        fh.write(struct.pack("<2i", 0, 1))


def test_ply_mesh_binary_quads_and_extra_properties(tmp_path):
    V, _ = MC.torus(nu=5, nv=4, with_normals=True)
    faces = [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9, 10, 11], [2, 1, 0]]
    want = np.array([[0, 1, 2], [3, 4, 5], [3, 5, 6], [7, 8, 9], [7, 9, 10], [7, 10, 11], [2, 1, 0]], dtype=np.int32)
    for extra in (True, False):
        path = str(tmp_path / f"b{int(extra)}.ply")
        _binary_ply(path, V, faces, extra=extra, index_name="vertex_index" if extra else "vertex_indices")
        V2, T2 = load_ply_mesh(path)
        assert V2.tobytes() == V.tobytes() and np.array_equal(T2, want) and T2.dtype == np.int32
    # the same in ASCII, with the extra column and a quad
    path = str(tmp_path / "a.ply")
    with open(path, "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty uchar red\nproperty float z\n"
                 "element face 1\nproperty list uchar uint vertex_indices\nend_header\n"
                 "0 0 255 0\n1 0 255 0.5\n1 1 255 0\n0 1 255 0.25\n4 0 1 2 3\n")
    V2, T2 = load_ply_mesh(path)
    assert V2.tolist() == [[0, 0, 0], [1, 0, 0.5], [1, 1, 0], [0, 1, 0.25]] and T2.tolist() == [[0, 1, 2], [0, 2, 3]]


def test_ply_mesh_errors_and_faceless_files(tmp_path):
    path = str(tmp_path / "cloud.ply")
    write_ply(MC.torus(nu=4, nv=3, with_normals=True)[0], path)     # a vertex list: no face element
    V, T = load_ply_mesh(path)
    assert V.shape == (12, 6) and T.shape == (0, 3) and T.dtype == np.int32
    bad = tmp_path / "bad.ply"
    for text, word in (("plx\n", "not a PLY"), ("ply\nformat binary_big_endian 1.0\nend_header\n", "binary_big_endian"),
                       ("ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n", "no vertex element"),
                       ("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                        "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n3 0 0 1\n", "face index"),
                       ("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n", ""),
                       ("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\n", "end_header")):
        bad.write_text(text)
        with pytest.raises(ValueError) as e:
            load_ply_mesh(str(bad))
        assert word in str(e.value)


# ---- C++ -------------------------------------------------------------------------------------------------------------------
FACADE_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "ppf_cloud_stages.hpp"
int main() {
  try {
    const float V[4 * 3] = {0.f, 0.f, 0.f, 0.05f, 0.f, 0.f, 0.f, 0.04f, 0.f, 0.05f, 0.04f, 0.03f};
    const int32_t T[2 * 3] = {0, 1, 2, 2, 1, 3};
    ppf_mesh_sample_params mp = ppfhip::prep::Cloud::defaultMeshSampleParams();
    mp.seed = 1;
    mp.map_size = 32;
    ppf_mesh_sample_stats st;
    const ppfhip::prep::Cloud a = ppfhip::prep::Cloud::fromMesh(V, 4, 3, -1, T, 2, &mp, &st);
    const ppfhip::prep::Cloud b = ppfhip::prep::Cloud::fromMesh(V, 4, 3, -1, T, 2);
    std::vector<float> rows, curv;
    a.download(rows, curv);
    std::printf("%d %lld %lld %lld %d %d %d\n", a.size(), (long long)st.n_sampled, (long long)st.n_rows, (long long)st.n_flipped, st.n_launches,
                st.n_host_syncs, b.size());
    return 0;
  } catch (const ppfhip::ppf_match_3d::Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 10 + (int)e.status;
  }
}
"""


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_the_cxx_facade_compiles_as_cxx11_and_runs(tmp_path, compiler):
    """prep::Cloud::fromMesh, warnings as errors; without a device the program ends with PPF_ERR_HIP's exit code, with one its
    counts are the oracle's"""
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
    V, T = MC.two_triangles()
    o = MO.mesh_sample(V, T, 0.004, seed=1, map_size=32)["stats"]
    d = MO.mesh_sample(V, T, 0.004)["stats"]
    assert [int(v) for v in r.stdout.split()] == [o["n_rows"], o["n_sampled"], o["n_rows"], o["n_flipped"], 17, 2, d["n_rows"]]


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_the_demo_is_cxx11(tmp_path, compiler):
    """examples/mesh_model_demo.cpp and the facade behind it, warnings as errors; a spacing of 0 is the library's refusal"""
    csrc = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
    exe = str(tmp_path / "mesh_model_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "mesh_model_demo.cpp"), "-L", csrc, "-lppf_hip", f"-Wl,-rpath,{csrc}", "-o", exe], check=True)
    r = subprocess.run([exe, "0"], capture_output=True, text=True)
    assert r.returncode == 10 + _capi.PPF_ERR_INVALID and "spacing" in r.stderr
    assert r.stdout.splitlines()[0] == "mesh 16 vertices 24 triangles spacing 0 seed 0 map 0"
