"""ppf_cloud_from_mesh on the device against tests/mesh_oracle.py: rows, counts and stats byte for byte (area to 1e-12), on the
smallest meshes where each path can go wrong -- one and two triangles, the box whose every draw takes the large path, the
torus whose every draw takes the small one, triangles below a pixel, the 16 | 17 pixel boundary between the paths, the largest
box a triangle can have, degenerate lists -- and the options, the capacity refusal of the device route, constant launches and
waits, the pool guard, two threads, and the wrappers: train and match, LoadMeshModel, the C++ demo."""
import ctypes as C
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import mesh_cases as MC
import mesh_oracle as MO
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
from yolo_ppf_pose_estimation_amd.ply import write_ply_mesh

pytestmark = pytest.mark.gpu

CASES = {
    "one triangle": (MC.one_triangle, dict(spacing=0.004, map_size=16)),
    "two triangles": (MC.two_triangles, dict(spacing=0.004, seed=1, map_size=32)),
    "box R64": (MC.box, dict(spacing=0.004, map_size=64)),
    "box-in-box R64": (MC.box_in_box, dict(spacing=0.004, map_size=64)),
    "box-in-box rotated R128": (lambda: MC.rotated(MC.box_in_box()), dict(spacing=0.004, map_size=128)),
    "torus 48x24 R128": (MC.torus, dict(spacing=0.003, map_size=128)),
    "torus 192x96 R16": (lambda: MC.torus(nu=192, nv=96), dict(spacing=0.003, map_size=16)),
    "16 pixels": (lambda: MC.boundary_triangle(16), dict(spacing=0.002, map_size=64)),
    "17 pixels": (lambda: MC.boundary_triangle(17), dict(spacing=0.002, map_size=64)),
    "lone triangle R512": (MC.lone_triangle, dict(spacing=0.004, map_size=512)),
    "lone triangle default R": (MC.lone_triangle, dict(spacing=0.01)),
    "degenerate list": (MC.degenerate_list, dict(spacing=0.002, map_size=64)),
    "all degenerate": (MC.all_degenerate, dict(spacing=0.002, map_size=64)),
    "vertex normals": (lambda: MC.torus(nu=24, nv=12, with_normals=True, vstride=8, normal_offset=4),
                       dict(spacing=0.003, map_size=64, normals=1, normal_offset=4)),
    "visibility off": (MC.box_in_box, dict(spacing=0.004, visibility=0, orient=0)),
    "min_views 3": (MC.box_in_box, dict(spacing=0.005, map_size=64, min_views=3)),
    "min_views 13": (MC.torus, dict(spacing=0.004, map_size=64, min_views=13)),
    "min_views 26": (MC.torus, dict(spacing=0.004, map_size=64, min_views=26)),
    "depth_tol 1 mm": (MC.box_in_box, dict(spacing=0.005, map_size=128, depth_tol=0.001)),
    "no orient": (MC.box_in_box, dict(spacing=0.005, map_size=64, orient=0)),
    "seed 7": (MC.box, dict(spacing=0.004, map_size=64, seed=7)),
    "seed 2^32 - 1": (MC.box, dict(spacing=0.004, map_size=64, seed=0xFFFFFFFF)),
}


@functools.lru_cache(maxsize=None)
def want(name):
    mesh, kw = CASES[name]
    V, T = mesh()
    kw = dict(kw)
    return V, T, MO.mesh_sample(V, T, kw.pop("spacing"), **kw)


def sample(V, T, kw):
    kw = dict(kw)
    normals = "vertex" if kw.pop("normals", 0) else "face"
    return DeviceCloud.from_mesh(V, T, kw.pop("spacing"), normals=normals, visibility=bool(kw.pop("visibility", 1)),
                                 orient=bool(kw.pop("orient", 1)), return_stats=True, **kw)


def check_case(name):
    V, T, o = want(name)
    cloud, st = sample(V, T, CASES[name][1])
    rows, curv = cloud.download()
    for f in ("n_triangles", "n_degenerate", "n_sampled", "n_hidden", "n_flipped", "n_rows", "n_large"):
        assert st[f] == o["stats"][f], (name, f, st[f], o["stats"][f])
    assert len(cloud) == len(o["rows"]) and rows.tobytes() == o["rows"].tobytes(), name
    assert not curv.any()
    assert abs(st["area"] - o["stats"]["area"]) <= 1e-12 * max(o["stats"]["area"], 1e-300) or st["area"] == o["stats"]["area"]
    assert (st["n_launches"], st["n_host_syncs"]) == ((17, 2) if CASES[name][1].get("visibility", 1) else (8, 2))
    assert st["reserved"] == [0, 0, 0, 0]
    return st


@pytest.mark.parametrize("name", list(CASES))
def test_rows_and_stats_equal_the_oracle(name):
    check_case(name)


def test_the_cases_take_the_paths_they_are_named_for():
    """what makes the cases above the smallest that matter, asserted on the oracle's own figures"""
    o = want("box R64")[2]
    assert o["stats"]["n_large"] == (o["sides"].max(axis=2) > 0).sum() > 100 and 7000 < o["stats"]["n_rows"] < 8500
    assert want("torus 48x24 R128")[2]["stats"]["n_large"] == 0
    o = want("torus 192x96 R16")[2]
    assert o["sides"].max() <= 2 and o["stats"]["n_large"] == 0 and (o["sides"].max(axis=2) == 0).mean() > 0.5
    assert want("16 pixels")[2]["sides"][13, 2, 0] == 16 and want("17 pixels")[2]["sides"][13, 2, 0] == 17
    assert want("16 pixels")[2]["stats"]["n_large"] == 0 and want("17 pixels")[2]["stats"]["n_large"] > 0
    assert want("lone triangle R512")[2]["sides"].max() > 350
    assert want("all degenerate")[2]["stats"]["n_sampled"] == 0 and want("degenerate list")[2]["stats"]["n_degenerate"] == 6
    o = want("box-in-box R64")[2]
    assert o["stats"]["n_hidden"] > 2000 and o["stats"]["n_flipped"] > 3000
    assert 1000 < want("min_views 13")[2]["stats"]["n_rows"] < want("min_views 13")[2]["stats"]["n_sampled"] - 1000
    assert want("min_views 26")[2]["stats"]["n_rows"] == 0 < want("min_views 26")[2]["stats"]["n_sampled"]  # no view sees all of a torus
    assert want("seed 7")[2]["rows"].tobytes() != want("box R64")[2]["rows"].tobytes()
    o = want("vertex normals")[2]
    face = MO.mesh_sample(*want("vertex normals")[:2], 0.003, map_size=64)
    assert o["rows"][:, :3].tobytes() == face["rows"][:, :3].tobytes() and o["rows"][:, 3:].tobytes() != face["rows"][:, 3:].tobytes()


def test_max_rows_on_the_device_route():
    V, T = MC.torus()
    assert len(T) > _capi.PPF_MESH_HOST_COUNT
    for kw in (dict(max_rows=5000), dict(max_rows=2)):  # the sum, and one triangle's q alone
        with pytest.raises(_capi.PPFError) as e:
            DeviceCloud.from_mesh(V, T, 0.003, map_size=64, **kw)
        assert e.value.status == _capi.PPF_ERR_CAPACITY and "max_rows" in str(e.value)
    st = _capi.MeshSampleStats()
    st.n_rows = 5
    out, prm = C.c_void_p(123), _capi.MeshSampleParams()
    _capi.lib().ppf_default_mesh_sample_params(C.byref(prm))
    prm.spacing, prm.max_rows = 0.003, 5000
    Vc, Tc = np.ascontiguousarray(V), np.ascontiguousarray(T)
    assert _capi.lib().ppf_cloud_from_mesh(Vc.ctypes.data, len(Vc), 3, -1, Tc.ctypes.data, len(Tc), C.byref(prm), C.byref(out),
                                           C.byref(st)) == _capi.PPF_ERR_CAPACITY
    assert not out.value and bytes(st) == bytes(len(bytes(st)))
    n = MO.mesh_sample(V, T, 0.003, visibility=0, orient=0)["stats"]["n_sampled"]
    assert len(DeviceCloud.from_mesh(V, T, 0.003, map_size=64, max_rows=n)) == n  # exactly max_rows is allowed


def test_launches_and_waits_do_not_depend_on_the_mesh():
    seen = {(check_case(n)["n_launches"], check_case(n)["n_host_syncs"]) for n in ("all degenerate", "torus 48x24 R128", "box R64")}
    assert seen == {(17, 2)}


@pytest.mark.parametrize("mode", [1, 2])
def test_under_the_pool_guard(mode):
    from test_gpu_pool_guard import run_guarded
    for name in ("box-in-box R64", "torus 48x24 R128", "17 pixels", "visibility off", "all degenerate"):
        run_guarded(mode, check_case, name)


def test_twice_and_from_two_threads():
    first = check_case("box-in-box R64")
    first.pop("area")
    again = check_case("box-in-box R64")
    again.pop("area")
    assert again == first
    errors = []

    def work(name):
        try:
            for _ in range(2):
                check_case(name)
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    for n in ("box-in-box R64", "torus 48x24 R128"):
        want(n)
    threads = [threading.Thread(target=work, args=(n,)) for n in ("box-in-box R64", "torus 48x24 R128")]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_sample_train_match():
    """a smoke check of the loop, no accuracy claim: the sampled box-in-box trained on, one side of it matched"""
    V, T = MC.box_in_box()
    model = DeviceCloud.from_mesh(V, T, 0.004).rows()
    assert len(model) > 7000 and np.isfinite(model).all()
    det = PPF3DDetector(0.05, 0.05)
    det.trainModel(model)
    view = np.array([0.5, 0.6, 0.62])
    scene = model[model[:, 3:].astype(np.float64) @ view > 0.1][::3].copy()
    scene[:, :3] += np.array([0.1, -0.05, 0.6], dtype=np.float32)
    poses = det.match(scene, 1.0 / 10.0, 0.05)
    assert len(poses) >= 1


def test_load_mesh_model_from_a_ply(tmp_path):
    V, T = MC.rotated(MC.box_in_box())
    path = str(tmp_path / "box.ply")
    write_ply_mesh(V, T, path)
    cp = CloudProcessor(None, None, [], [], [], 0.05, 0.05)
    st = cp.LoadMeshModel(path, "box")
    ext = V.astype(np.float64).max(axis=0) - V.astype(np.float64).min(axis=0)
    spacing = 0.5 * 0.05 * float(np.linalg.norm(ext))
    o = MO.mesh_sample(V, T, spacing)
    ref = CloudProcessor(None, None, [], [], [], 0.05, 0.05)
    ref.LoadSingleModel(o["rows"], "box")
    assert cp.models[0].tobytes() == ref.models[0].tobytes() and cp.models[0].dtype == ref.models[0].dtype
    assert cp.label_to_id == ref.label_to_id and cp.if_trained == [False] and st["n_rows"] == len(o["rows"])
    st2 = cp.LoadMeshModel((V, T), "again", spacing=0.004, map_size=64)
    assert st2["n_rows"] == len(cp.models[1]) == MO.mesh_sample(V, T, 0.004, map_size=64)["stats"]["n_rows"]


def test_cpp_demo_matches_the_python_route(tmp_path):
    """examples/mesh_model_demo.cpp: the stats and the digest of the rows it prints are the Python route's on its mesh"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "yolo_ppf_pose_estimation_amd", "csrc")
    exe = str(tmp_path / "mesh_model_demo")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "mesh_model_demo.cpp"), "-L", csrc, "-lppf_hip", f"-Wl,-rpath,{csrc}", "-o", exe], check=True)
    r = subprocess.run([exe, "0.004", "3", "64"], check=True, capture_output=True, text=True, timeout=120)
    V, T = MC.box_in_box()
    cloud, st = DeviceCloud.from_mesh(V, T, 0.004, seed=3, map_size=64, return_stats=True)
    h = 14695981039346656037
    for b in cloud.rows().tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    lines = [f"mesh {len(V)} vertices {len(T)} triangles spacing 0.004 seed 3 map 64",
             f"triangles {st['n_triangles']} degenerate {st['n_degenerate']} sampled {st['n_sampled']} hidden {st['n_hidden']} "
             f"flipped {st['n_flipped']} rows {st['n_rows']} large {st['n_large']}",
             f"launches {st['n_launches']} waits {st['n_host_syncs']} area {st['area']:.9f}",
             f"digest {h:016x}"]
    assert r.stdout.splitlines() == lines, r.stdout
