"""ppf_depth_volume_mesh and ppf_depth_volume_write on the device against tests/volume_mesh_oracle.py, byte for byte: vertices,
triangles and all four counts, on integrated box volumes and on random volumes written into the device volume -- one cube,
odd sizes, a row longer than a tile, vertex references across tiles, and the volume that reaches all 84 non-empty
(tetrahedron, case) pairs -- at min_weight 1 and 2; empty results; write against read, integrate and extract; determinism, two
threads, the pool guard, constant launches and waits; the loop scan -> mesh -> PLY -> LoadMeshModel -> train -> match; and
the C++ demo against the Python route.  No test provokes a failing launch."""
import os
import subprocess
import threading

import numpy as np
import pytest

import depth_volume_cases as VC
import depth_volume_oracle as O
import volume_mesh_oracle as M
from test_gpu_depth_volume import integrate_both, make, same_voxels
from test_volume_mesh_oracle import CASES_VOLUME
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DepthVolume, DeviceCloud
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector

pytestmark = pytest.mark.gpu
cases = O.cases
F32 = np.float32
BOX_DIMS = [(1, 1, 1), (2, 3, 5), (7, 5, 3), (33, 9, 6), (8, 8, 8)]
RANDOM = [((2, 2, 2), 4), ((3, 3, 3), 1), ((5, 4, 3), 3), CASES_VOLUME, ((257, 2, 2), 2), ((33, 9, 6), 4)]
KINDS = ["identity", "moved", "behind", "aside", "moved"]


def mesh_both(dv, ov, min_weight=1, what=""):
    m, st = dv.mesh(dict(min_weight=min_weight), return_stats=True)
    wv, wt, wst = M.mesh(ov, min_weight)
    assert {k: st[k] for k in wst} == wst, (what, st, wst)
    v, t = m.vertices(), m.triangles()
    assert (m.n_vertices, m.n_triangles) == (len(wv), len(wt)) and v.shape == wv.shape and t.shape == wt.shape, what
    assert t.dtype == np.int32 and t.tobytes() == wt.tobytes(), (what, "triangles", int((t != wt).any(axis=1).sum()))
    assert v.dtype == F32 and v.tobytes() == wv.tobytes(), (what, "vertices", int((v.view(np.int32) != wv.view(np.int32)).any(axis=1).sum()))
    return wst


def written(ov):
    """a device volume holding the records of the oracle volume ov"""
    dv = DepthVolume(**M.volume_params(ov))
    dv.write(ov.d, ov.w)
    return dv


def box(dims, n_frames=4):
    """a volume of `dims` filled from four posed frames, as test_gpu_depth_volume.check_box fills one"""
    vp = VC.box_volume(dims)
    dv, ov = make(vp)
    for f in range(n_frames):
        img, intr = VC.box_frame(vp, 24, 40, seed=f)
        integrate_both(dv, ov, img, intr, VC.box_pose(vp, KINDS[f % len(KINDS)], seed=f), what=f"{dims} frame {f}", z_min=0.2, z_max=3.0)
    return dv, ov


def check_box_mesh(dims):
    dv, ov = box(dims)
    return [mesh_both(dv, ov, mw, what=f"box {dims} min_weight {mw}") for mw in (1, 2)]


def check_random_mesh(dims, seed):
    ov = M.random_volume(dims, seed)
    dv = written(ov)
    return [mesh_both(dv, ov, mw, what=f"random {dims} min_weight {mw}") for mw in (1, 2)]


@pytest.mark.parametrize("dims", BOX_DIMS, ids=[str(d) for d in BOX_DIMS])
def test_integrated_box_volumes(dims):
    st = check_box_mesh(dims)
    if dims == (1, 1, 1):
        assert st[0]["n_cells"] == 0 and st[0]["n_triangles"] == 0 and st[0]["n_vertices"] == 0
    if dims == (2, 3, 5):   # three active cubes at weight 1, none at weight 2: an empty mesh
        assert st[0]["n_triangles"] > 0 and st[1]["n_cells"] == 0 and st[1]["n_triangles"] == 0 and st[1]["n_vertices"] == 0
    if dims in ((33, 9, 6), (8, 8, 8), (7, 5, 3)):
        assert st[0]["n_triangles"] > 0 and st[0]["n_cells"] > 0


@pytest.mark.parametrize("dims,seed", RANDOM, ids=[str(d) for d, _ in RANDOM])
def test_random_volumes_through_write(dims, seed):
    st = check_random_mesh(dims, seed)
    assert st[0]["n_cells"] > 0 and st[0]["n_triangles"] > 0, st
    if dims in ((33, 9, 6), (257, 2, 2)):
        assert st[1]["n_triangles"] > 0
    if dims == (33, 9, 6):
        assert 0 < st[0]["n_no_normal"] < st[0]["n_vertices"]


def test_the_sphere_at_64_cubed():
    dv, ov = make(VC.SPHERE_VOLUME)
    intr = cases.intrinsics()
    for f, T in zip(VC.sphere_frames(), VC.SPHERE_VIEWS):
        integrate_both(dv, ov, f, intr, T, what="sphere")
    st = mesh_both(dv, ov, what="sphere mesh")
    assert st["n_triangles"] > 20000


def test_empty_and_all_negative_volumes_give_an_empty_mesh():
    vp = VC.box_volume((8, 8, 8))
    dv, ov = make(vp)
    for what in ("empty", "negative"):
        if what == "negative":
            ov.d[...], ov.w[...] = F32(-0.5), 2
            dv.write(ov.d, ov.w)
        m, st = dv.mesh(return_stats=True)
        assert (m.n_vertices, m.n_triangles, st["n_vertices"], st["n_triangles"], st["n_no_normal"]) == (0, 0, 0, 0, 0), what
        assert st["n_cells"] == (343 if what == "negative" else 0) and (st["n_launches"], st["n_host_syncs"]) == (M.N_LAUNCHES, M.N_HOST_SYNCS)
        assert m.vertices().shape == (0, 6) and m.triangles().shape == (0, 3)
        mesh_both(dv, ov, what=what)


def test_info_and_read_check_their_arguments():
    """the counts must be the mesh's and a buffer may only be NULL when its count is 0: refused in that order, nothing written"""
    import ctypes as C
    lib = _capi.lib()
    m = written(M.random_volume((5, 4, 3), 3)).mesh()
    nv, nt = m.n_vertices, m.n_triangles
    d = _capi.VolumeMeshDesc()
    _capi.check(lib.ppf_volume_mesh_info(m._ptr, C.byref(d)))
    assert (d.n_vertices, d.n_triangles) == (nv, nt) and nv > 0 and nt > 0 and d.device_bytes >= nv * 24 + nt * 12
    assert lib.ppf_volume_mesh_info(m._ptr, None) == _capi.PPF_ERR_INVALID
    v, t = np.full((nv, 6), 7.0, F32), np.full((nt, 3), 7, np.int32)
    read = lambda vp, n_v, tp, n_t: lib.ppf_volume_mesh_read(m._ptr, vp, n_v, tp, n_t)
    for n_v, n_t in ((nv - 1, nt), (nv, nt + 1), (0, 0)):
        assert read(None, n_v, None, n_t) == _capi.PPF_ERR_INVALID and f"the mesh has {nv} and {nt}" in _capi.last_error()
    assert read(None, nv, t.ctypes.data, nt) == _capi.PPF_ERR_INVALID and "vertices is NULL" in _capi.last_error()
    assert read(v.ctypes.data, nv, None, nt) == _capi.PPF_ERR_INVALID and "triangles is NULL" in _capi.last_error()
    assert (v == 7.0).all() and (t == 7).all()
    assert read(v.ctypes.data, nv, t.ctypes.data, nt) == _capi.PPF_OK
    assert v.tobytes() == m.vertices().tobytes() and t.tobytes() == m.triangles().tobytes()


def test_write_round_trip_then_integrate_and_extract():
    ov = M.random_volume((33, 9, 6), 7, max_weight=64)
    dv = written(ov)
    same_voxels(dv, ov, "write -> read")
    assert dv.info()["integrations"] == 0
    want, wst = O.extract(ov, 1)
    cloud, st = dv.extract(return_stats=True)
    assert {k: st[k] for k in wst} == wst and cloud.download()[0].tobytes() == want.tobytes() and wst["n_rows"] > 0
    vp = M.volume_params(ov)
    img, intr = VC.box_frame(vp, 24, 40, seed=1)
    assert integrate_both(dv, ov, img, intr, np.eye(4), what="write -> integrate") > 0
    assert dv.info()["integrations"] == 1
    mesh_both(dv, ov, what="write -> integrate -> mesh")
    # a refused write leaves the volume alone
    before = dv.read()
    bad = ov.d.copy()
    bad[2, 3, 4] = np.nan
    with pytest.raises(_capi.PPFError) as e:
        dv.write(bad, ov.w)
    assert e.value.status == _capi.PPF_ERR_INVALID and f"record {(2 * 9 + 3) * 33 + 4} " in str(e.value)
    after = dv.read()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()


def test_twice_and_from_two_threads():
    first = check_random_mesh((33, 9, 6), 4)
    assert check_random_mesh((33, 9, 6), 4) == first
    ov = M.random_volume((33, 9, 6), 4)
    dv = written(ov)
    a, b = dv.mesh(), dv.mesh()
    assert a.vertices().tobytes() == b.vertices().tobytes() and a.triangles().tobytes() == b.triangles().tobytes()
    errors = []

    def work(dims, seed):
        try:
            for _ in range(2):
                check_random_mesh(dims, seed)
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=a) for a in (((33, 9, 6), 4), CASES_VOLUME)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("mode", [1, 2])
def test_the_helpers_under_the_pool_guard(mode):
    from test_gpu_pool_guard import run_guarded
    run_guarded(mode, check_random_mesh, (33, 9, 6), 4)
    run_guarded(mode, check_box_mesh, (7, 5, 3))


def test_launches_and_syncs_do_not_depend_on_the_volume():
    seen = set()
    empty = make(VC.box_volume((8, 8, 8)))[0]
    for dv in (empty, box((8, 8, 8))[0], written(M.random_volume((8, 8, 8), 0))):
        st = dv.mesh(return_stats=True)[1]
        seen.add((st["n_launches"], st["n_host_syncs"]))
    assert seen == {(M.N_LAUNCHES, M.N_HOST_SYNCS)}


def scan():
    dv = make(VC.SPHERE_VOLUME)[0]
    intr = cases.intrinsics()
    for T in VC.SPHERE_VIEWS:
        dv.integrate(VC.render_scan(T), intr, T)
    return dv, intr


def test_scan_mesh_ply_train_match(tmp_path):
    """a smoke check of the loop, no accuracy claim: a sphere and an ellipsoid scanned from four sides, the mesh saved as a PLY,
    loaded as a mesh model, trained on, and one view of them matched"""
    dv, intr = scan()
    m = dv.mesh()
    path = str(tmp_path / "scan.ply")
    m.save_ply(path)
    cp = CloudProcessor(None, VC.render_scan(VC.SPHERE_VIEWS[0]), [], [], [], 0.05, 0.05)
    stats = cp.LoadMeshModel(path, "scan", normals="vertex", orient=False)
    model = cp.models[0]
    assert m.n_triangles > 10000 and len(model) > 0 and np.isfinite(model).all(), stats
    det = PPF3DDetector(0.05, 0.05)
    det.trainModel(model)
    scene = DeviceCloud.from_depth(VC.render_scan(VC.SPHERE_VIEWS[1]), intr, normals=dict(drop=True)).rows()
    assert len(det.match(scene, 1.0 / 10.0, 0.05)) >= 1


def test_mesh_volume_of_the_processor(tmp_path):
    """CloudProcessor.MeshVolume: refused before FuseVolume, then the mesh of the fused volume, written where asked"""
    from yolo_ppf_pose_estimation_amd.ply import load_ply_mesh
    frames, _ = cases.stream(2, 5, 20.0, 2.0)
    cp = CloudProcessor(None, frames[0], [], [], [], 0.05, 0.05)
    with pytest.raises(_capi.PPFError) as e:
        cp.MeshVolume()
    assert e.value.status == _capi.PPF_ERR_INVALID and "FuseVolume" in str(e.value)
    vol = make(VC.SCENE_VOLUME)[0]
    ora = O.Fusion(VC.SHAPE, cases.intrinsics(), O.Volume(**VC.SCENE_VOLUME), raycast_params=VC.SCENE_RAYCAST)
    for f in frames:
        cp.FuseVolume(f, CameraIntr=cases.intrinsics(), **(dict(volume=vol, raycast_params=VC.SCENE_RAYCAST) if f is frames[0] else {}))
        ora.push(f)
    path = str(tmp_path / "scene.ply")
    m = cp.MeshVolume(path)
    wv, wt, _ = M.mesh(ora.vol, 1)
    assert m.vertices().tobytes() == wv.tobytes() and m.triangles().tobytes() == wt.tobytes() and len(wt) > 0
    pv, pt = load_ply_mesh(path)
    assert pv.shape == wv.shape and np.array_equal(pt, wt) and "mesh_volume" in cp.timings


def test_cpp_demo_matches_the_python_route(tmp_path):
    """examples/volume_mesh_demo.cpp on the four scan views: its counts, the digests of its mesh and the rows it samples are the
    Python route's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "yolo_ppf_pose_estimation_amd", "csrc")
    exe = str(tmp_path / "volume_mesh_demo")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "volume_mesh_demo.cpp"), "-L", csrc, "-lppf_hip", f"-Wl,-rpath,{csrc}", "-o", exe], check=True)
    intr, vp, spacing = cases.intrinsics(), VC.SPHERE_VOLUME, 0.004
    frames = [VC.render_scan(T) for T in VC.SPHERE_VIEWS]
    np.concatenate([f.reshape(-1) for f in frames]).astype("<f4").tofile(str(tmp_path / "frames.f32"))
    np.concatenate([np.asarray(T, np.float64).reshape(-1) for T in VC.SPHERE_VIEWS]).astype("<f8").tofile(str(tmp_path / "poses.f64"))
    args = ([str(tmp_path / "frames.f32"), str(tmp_path / "poses.f64"), str(len(frames)), str(VC.SHAPE[0]), str(VC.SHAPE[1])] +
            [repr(float(v)) for v in intr] + [str(d) for d in vp["dims"]] + [repr(float(F32(vp["voxel"])))] +
            [repr(float(v)) for v in vp["origin"]] + [repr(float(F32(vp["trunc"]))), repr(float(F32(spacing)))])
    r = subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=120)
    dv = make(vp)[0]
    want = [f"frame {k} updated {dv.integrate(f, intr, T)}" for k, (f, T) in enumerate(zip(frames, VC.SPHERE_VIEWS))]
    m, st = dv.mesh(return_stats=True)
    v, t = m.vertices(), m.triangles()
    want += [f"mesh vertices {len(v)} triangles {len(t)} cells {st['n_cells']} without a normal {st['n_no_normal']}",
             f"digest vertices {M.fnv1a(v.tobytes()):016x} triangles {M.fnv1a(t.tobytes()):016x}"]
    rows = DeviceCloud.from_mesh(v, t, float(F32(spacing)), normals="vertex", orient=False).rows()
    want += [f"sampled rows {len(rows)} digest {M.fnv1a(rows.tobytes()):016x}"]
    assert r.stdout.splitlines() == want, r.stdout
    assert len(t) > 10000 and len(rows) > 1000
