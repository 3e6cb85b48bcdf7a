"""ppf_prep_frame: every detection of a frame prepared in one segmented device pass.  Each box's object and edge clouds
are bit-identical to the single-box ppf_prep_* chain (crop -> voxel grid -> outlier removal -> normals -> edges ->
to-Mat), on the reference's frame and on seeded draws; the launch and host-sync counts do not depend on the number of
boxes; errors leave no handle; outputs outlive their siblings; PrepareFrame + MatchFrame give the per-box route's poses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import prep_data as D
from yolo_ppf_pose_estimation_amd import _capi, synth
from yolo_ppf_pose_estimation_amd._capi import FrameParams, FrameStats, PPFError, lib
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
DEFAULTS = dict(leaf=0.003, mean_k=50, stddev_mul=1.0, normal_k=30, curvature_threshold=0.03)


@pytest.fixture(scope="module")
def frame():
    return D.c1_frame()


def per_box(scene, box, depth, intr, p):
    c = scene.crop(box, depth, intr)
    v = c.voxel_grid(p["leaf"])
    o = v.outlier_removal(p["mean_k"], p["stddev_mul"])
    n = o.normals(p["normal_k"])
    e = n.edges(p["curvature_threshold"])
    return n.to_mat().download(), e.to_mat().download(), [len(c), len(v), len(o), len(e)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want):
    assert got[0].shape == want[0].shape
    np.testing.assert_array_equal(bits(got[0]), bits(want[0]))
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]))


def check_frame(scene, boxes, depth, intr, p):
    pairs, rows, stats = scene.prep_frame(boxes, depth, intr, p, return_info=True)
    assert len(pairs) == len(boxes) and stats["n_host_syncs"] <= 3
    for i, b in enumerate(boxes):
        wo, we, wrows = per_box(scene, b, depth, intr, p)
        assert list(rows[i]) == wrows, (i, b)
        assert_same(pairs[i][0].download(), wo)
        assert_same(pairs[i][1].download(), we)
    return pairs, rows, stats


def frame_boxes(frame):
    _, depth, (x, y, w, h), _ = frame
    H, W = depth.shape
    return [(x, y, w, h), (x - 40, y, w, h), (x + 40, y, w, h), (x + 20, y + 20, w, h), (x - 10, y - 15, w + 30, h + 25),
            (W - 1 - w // 2, y, w // 2, h), (5, 5, 10, 10), (x, y, w, h)]


def test_real_frame_every_box_bitwise(frame):
    xyz, depth, box, intr = frame
    scene = DeviceCloud.upload(xyz)
    boxes = frame_boxes(frame)
    pairs, rows, _ = check_frame(scene, boxes, depth, intr, DEFAULTS)
    assert list(rows[0]) == [35749, 11369, 10395, 1447]          # c1_pipeline_golden.npz, DESIGN §11
    assert list(rows[6]) == [0, 0, 0, 0] and len(pairs[6][0]) == 0   # the empty corner
    assert list(rows[7]) == list(rows[0])                          # the duplicate
    # the fixture box against the CPU prep oracle
    keep, _ = O.prep_crop(xyz, box, depth, intr)
    want = O.prep_voxel(xyz[keep], 0.003)
    k2, _, _ = O.prep_sor(want, 50, 1.0)
    want = want[k2]
    n, c = O.prep_normals(want, 30)
    r0, c0 = pairs[0][0].download()
    np.testing.assert_array_equal(r0, O.prep_to_mat(want, n))
    np.testing.assert_array_equal(c0, c)
    np.testing.assert_array_equal(pairs[0][1].rows(), O.prep_to_mat(want[c > 0.03], n[c > 0.03]))


def _voxel_volume(pts, leaf):
    if pts.shape[0] == 0:
        return 0
    inv = np.float32(1.0) / np.float32(leaf)
    lo = np.floor(pts.min(axis=0) * inv).astype(np.int64)
    hi = np.floor(pts.max(axis=0) * inv).astype(np.int64)
    return int(np.prod(hi - lo + 1))


@pytest.mark.parametrize("seed", range(20))
def test_seeded_draws_every_segment_bitwise(frame, seed):
    rng = np.random.default_rng(7100 + seed)
    fxyz, depth, (x0, y0, w0, h0), intr = frame
    H, W = depth.shape
    xyz = fxyz.copy()
    bad = rng.integers(0, xyz.shape[0], 20)
    xyz[bad[:10]] = [np.nan, 0.0, 1.0]
    xyz[bad[10:]] = [0.0, np.inf, 0.5]
    scene = DeviceCloud.upload(xyz)
    K = int(rng.integers(1, 17))
    boxes = []
    for _ in range(K):
        kind = rng.integers(0, 4)
        if kind == 0:     # around the object
            bx, by, bw, bh = x0 + rng.integers(-60, 60), y0 + rng.integers(-60, 60), w0 + rng.integers(-80, 80), h0 + rng.integers(-80, 80)
        elif kind == 1:   # tiny: segments with n <= meanK and n < k
            bx, by, bw, bh = x0 + rng.integers(0, w0), y0 + rng.integers(0, h0), rng.integers(0, 4), rng.integers(0, 4)
        elif kind == 2:   # beside / across, touching the border
            bx, by, bw, bh = rng.integers(0, W - 2), rng.integers(0, H - 2), rng.integers(2, 500), rng.integers(2, 400)
        else:             # outside the object
            bx, by, bw, bh = rng.integers(0, 60), rng.integers(0, 60), rng.integers(2, 40), rng.integers(2, 40)
        bx, by = int(max(0, min(bx, W - 2))), int(max(0, min(by, H - 2)))
        boxes.append((bx, by, int(max(0, min(bw, W - 1 - bx))), int(max(0, min(bh, H - 1 - by)))))
    p = dict(leaf=float(rng.choice([0.002, 0.003, 0.005, 0.011])), mean_k=int(rng.integers(2, 64)),
             stddev_mul=float(rng.choice([0.5, 1.0, 2.0])), normal_k=int(rng.integers(1, 65)),
             curvature_threshold=float(rng.choice([0.01, 0.03, 0.08])))
    if seed == 0:
        # a leaf small enough that the boxes' voxel volumes add up past 2^32 while each stays below 2^31
        boxes = [(x0 + 10 * i, y0 + 10 * i, w0 // 3, h0 // 3) for i in range(16)]
        crops = [xyz[O.prep_crop(xyz, b, depth, intr)[0]] for b in boxes]
        crops = [c[np.isfinite(c).all(axis=1)] for c in crops]
        for leaf in (0.0002, 0.0003, 0.0004, 0.0005, 0.0007, 0.001):
            vols = [_voxel_volume(c, leaf) for c in crops]
            if max(vols) < 2 ** 31 and sum(vols) > 2 ** 32:
                break
        else:
            pytest.fail(f"no leaf gives the wanted volumes: {vols}")
        p["leaf"] = leaf
    check_frame(scene, boxes, depth, intr, p)


def test_launches_and_syncs_do_not_depend_on_the_box_count(frame):
    xyz, depth, box, intr = frame
    scene = DeviceCloud.upload(xyz)
    boxes = (frame_boxes(frame)[:6] * 3)[:16]
    _, _, s1 = scene.prep_frame(boxes[:1], depth, intr, DEFAULTS, return_info=True)
    _, _, s16 = scene.prep_frame(boxes, depth, intr, DEFAULTS, return_info=True)
    assert s1["n_boxes"] == 1 and s16["n_boxes"] == 16
    assert s1["n_host_syncs"] <= 3 and s1["n_host_syncs"] == s16["n_host_syncs"]
    assert s1["n_launches"] == s16["n_launches"] > 0
    pairs, _, s0 = scene.prep_frame(np.zeros((0, 4), np.int32), depth, intr, DEFAULTS, return_info=True)
    assert pairs == [] and s0["n_launches"] == 0


def test_the_waits_of_a_call_are_three_and_two_when_no_box_holds_a_point(frame):
    """crop, voxel grid, the end; a frame whose boxes crop nothing stops after the crop's read-back and ends like every call"""
    xyz, depth, box, intr = frame
    boxes = frame_boxes(frame)[:3]
    _, _, st = DeviceCloud.upload(xyz).prep_frame(boxes, depth, intr, DEFAULTS, return_info=True)
    assert st["n_host_syncs"] == 3
    far = DeviceCloud.upload(xyz[:1000] + np.float32([1000.0, 0.0, 0.0]))
    pairs, rows, st = far.prep_frame(boxes, depth, intr, DEFAULTS, return_info=True)
    assert (st["n_host_syncs"], st["n_launches"]) == (2, 6) and not np.asarray(rows).any()      # k_frame_crop_flags and one scan
    assert all(len(o) == 0 and len(e) == 0 for o, e in pairs)


def _raw_frame(scene, boxes, depth, intr, p):
    b = np.ascontiguousarray(np.asarray(boxes, np.int32))
    prm = FrameParams()
    lib().ppf_default_frame_params(C.byref(prm))
    for k, v in p.items():
        setattr(prm, k, v)
    it = (C.c_double * 4)(*intr)
    objs, edges = (C.c_void_p * len(boxes))(*([0x1234] * len(boxes))), (C.c_void_p * len(boxes))(*([0x1234] * len(boxes)))
    s = lib().ppf_prep_frame(scene._ptr, b.ctypes.data_as(C.POINTER(C.c_int)), len(boxes), depth.ctypes.data, depth.shape[0],
                             depth.shape[1], it, C.byref(prm), objs, edges, None, None)
    return s, objs, edges


def test_voxel_overflow_names_the_box_and_leaves_no_handle(frame):
    xyz, depth, (x0, y0, w0, h0), intr = frame
    scene = DeviceCloud.upload(xyz)
    boxes = [(x0 + 5 * i, y0 + 5 * i, 2, 2) for i in range(5)]
    boxes[3] = (x0, y0, w0, h0)
    crops = [xyz[O.prep_crop(xyz, b, depth, intr)[0]] for b in boxes]
    leaf = next(lf for lf in (1e-4, 5e-5, 2e-5, 1e-5)
                if _voxel_volume(crops[3], lf) > 2 ** 31 and all(_voxel_volume(c, lf) < 2 ** 31 for i, c in enumerate(crops) if i != 3))
    s, objs, edges = _raw_frame(scene, boxes, depth, intr, dict(DEFAULTS, leaf=leaf))
    assert s == _capi.PPF_ERR_INVALID
    assert "box 3" in _capi.last_error() and "overflow" in _capi.last_error()
    assert all(not o for o in objs) and all(not e for e in edges)
    with pytest.raises(PPFError):   # the single-box chain fails on the same box
        scene.crop(boxes[3], depth, intr).voxel_grid(leaf)
    # a box outside the depth image, and the next call still works
    bad = list(boxes)
    bad[2] = (depth.shape[1] + 100, 0, 10, 10)
    s, objs, _ = _raw_frame(scene, bad, depth, intr, DEFAULTS)
    assert s == _capi.PPF_ERR_INVALID and "box 2" in _capi.last_error() and all(not o for o in objs)
    check_frame(scene, boxes[2:4], depth, intr, DEFAULTS)


def test_outputs_survive_their_siblings(frame, bottle):
    from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
    xyz, depth, box, intr = frame
    scene = DeviceCloud.upload(xyz)
    boxes = frame_boxes(frame)
    want = [per_box(scene, b, depth, intr, DEFAULTS) for b in boxes]
    det = PPF3DDetector(0.05, 0.05).trainModel(bottle)
    mp = det._params(0.05, 0.05, False)

    def match(obj, edge):
        cap = len(obj) + 8
        out, n = (_capi.Pose * cap)(), C.c_int(0)
        _capi.check(lib().ppf_match_clouds(det._model.ptr, obj._ptr, edge._ptr, C.byref(mp), out, cap, C.byref(n)))
        return [bytes(out[i]) for i in range(n.value)]

    ref = match(DeviceCloud.upload(want[0][0][0]), DeviceCloud.upload(want[0][1][0]))
    for order in ("reverse", "shuffled"):
        pairs = scene.prep_frame(boxes, depth, intr, DEFAULTS)
        handles = [(i, w, c) for i, pr in enumerate(pairs) for w, c in enumerate(pr)]
        keep = handles.pop(0 if order == "reverse" else 1)            # box 0's object (reverse) or edge (shuffled) survives
        seq = handles[::-1] if order == "reverse" else [handles[j] for j in np.random.default_rng(3).permutation(len(handles))]
        for k, (i, w, c) in enumerate(seq):
            c.__del__()
            if k % 5 == 0:   # the survivor stays readable while its siblings go
                assert_same(keep[2].download(), want[keep[0]][keep[1]])
        assert_same(keep[2].download(), want[keep[0]][keep[1]])
        if order == "reverse":
            obj = keep[2]
            edge = DeviceCloud.upload(want[0][1][0])
            assert match(obj, edge) == ref
    pairs = scene.prep_frame(boxes[:1], depth, intr, DEFAULTS)
    assert match(pairs[0][0], pairs[0][1]) == ref


LAYOUT = ([0.02, 0.0, 0.62], [-0.22, 0.0, 0.62], [0.25, 0.02, 0.7])   # centres of the two bottles and the box


def _render_frame(bottle):
    rows, cols, fx, fy, ppx, ppy = 360, 640, 460.0, 460.0, 319.5, 179.5
    vv, uu = np.mgrid[0:rows, 0:cols]
    ray = np.stack([(uu - ppx) / fx, (vv - ppy) / fy, np.ones_like(uu, dtype=np.float64)], axis=-1)
    nrm, off = np.array([0.1, -0.15, -1.0]) / np.linalg.norm([0.1, -0.15, -1.0]), -0.95
    depth = (off / (ray @ nrm)).astype(np.float32)
    solid = synth.make_solid("box", 20000, seed=7)
    solid[:, :3] *= 0.5
    R = synth.random_rotation(np.random.default_rng(8))
    objs = []
    for model, shift in zip((bottle, bottle, solid), LAYOUT):
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = np.array(shift) - R @ model[:, :3].mean(axis=0)
        objs.append((model, T))
    boxes = []
    for model, T in objs:
        obj = synth.apply_pose(model, T)[:, :3].astype(np.float64)
        pu = np.round(obj[:, 0] / obj[:, 2] * fx + ppx).astype(int)
        pv = np.round(obj[:, 1] / obj[:, 2] * fy + ppy).astype(int)
        order = np.argsort(-obj[:, 2])                              # nearest written last (the objects do not overlap)
        for du in (0, 1):
            for dv in (0, 1):
                depth[np.clip(pv[order] + dv, 0, rows - 1), np.clip(pu[order] + du, 0, cols - 1)] = obj[order, 2]
        boxes.append((int(pu.min()), int(pv.min()), int(pu.max() - pu.min()), int(pv.max() - pv.min())))
    zz = depth.astype(np.float64)
    scene = np.stack([(uu - ppx) * zz / fx, (vv - ppy) * zz / fy, zz], axis=-1).reshape(-1, 3).astype(np.float32)
    K = np.array([[fx, 0, ppx], [0, fy, ppy], [0, 0, 1.0]])
    return scene, depth, boxes, K, objs, solid


def test_prepare_frame_then_match_frame_end_to_end(bottle):
    from scipy.spatial import cKDTree
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    labels = ["bottle", "bottle", "box"]
    cp = CloudProcessor(scene, depth, boxes, [39, 39, 73], [0, 1, 2], 0.05, 0.05)
    cp.LoadSingleModel(bottle, "bottle")
    cp.LoadSingleModel(solid, "box")
    cp.TrainDetector(0.05, 0.05)
    pairs = cp.PrepareFrame(K, 0.004, 50, 1.0, 30, 0.03)
    assert len(pairs) == 3 and cp.stage_rows.shape == (3, 4) and (cp.stage_rows[:, 3] > 0).all()
    poses = cp.MatchFrame(labels)
    assert cp.MatchFrame([None, None, None]) == [None, None, None]
    # the per-box route: the six stage calls per box, then Matching_S2B on the resident clouds
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    for i, (b, name) in enumerate(zip(boxes, labels)):
        c = cp.scene.crop(b, depth, intr).voxel_grid(0.004).outlier_removal(50, 1.0).normals(30)
        want = cp.Matching_S2B(name, c.to_mat(), c.edges(0.03).to_mat())
        if want is None:
            assert poses[i] is None
            continue
        np.testing.assert_array_equal(poses[i].pose, want.pose)
        assert (poses[i].numVotes, poses[i].residual) == (want.numVotes, want.residual)
    for i in (0, 1):   # each bottle lands on its own true pose
        model, T = objs[i]
        assert poses[i] is not None
        truth = cKDTree(synth.apply_pose(model[::4], T)[:, :3].astype(np.float64))
        d, _ = truth.query(synth.apply_pose(model[::4], poses[i].pose)[:, :3].astype(np.float64))
        assert d.mean() < 0.003, (i, d.mean())


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_cpp_facade_prepare_frame(tmp_path, frame, compiler):
    xyz, depth, box, intr = frame
    exe = str(tmp_path / "frame_stages_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frame_stages_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}",
                    "-o", exe], check=True)
    boxes = np.asarray(frame_boxes(frame), np.int32)
    (tmp_path / "scene.f32").write_bytes(np.ascontiguousarray(xyz, np.float32).tobytes())
    (tmp_path / "depth.f32").write_bytes(np.ascontiguousarray(depth, np.float32).tobytes())
    (tmp_path / "boxes.i32").write_bytes(boxes.tobytes())
    r = subprocess.run([exe, str(tmp_path / "scene.f32"), str(xyz.shape[0]), str(tmp_path / "depth.f32"), str(depth.shape[0]),
                        str(depth.shape[1])] + [repr(float(v)) for v in intr] +
                       ["0.003", "1.0", str(tmp_path / "boxes.i32"), str(len(boxes))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pairs, rows, stats = DeviceCloud.upload(xyz).prep_frame(boxes, depth, intr, DEFAULTS, return_info=True)
    lines = r.stdout.strip().splitlines()
    for i, (o, e) in enumerate(pairs):
        f = lines[i].split()
        assert f[0] == "box" and [int(v) for v in f[3:10:2]] == list(rows[i]), lines[i]
        assert (int(f[11]), int(f[13])) == (len(o), len(e))
    assert lines[-1] == f"launches {stats['n_launches']} host_syncs {stats['n_host_syncs']}"
