"""ppf_match_frame on the device: every detection's rows (pose, q, t, angle, residual, votes; ICP iterations) are
bit-identical to ppf_match_clouds + ppf_icp_refine_clouds on that detection alone, whatever the other detections of the
call are; the ICP launch count does not grow with the number of detections; the golden C1 chain; the flags; two
concurrent callers; the Python and C++ wrappers."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import prep_data as D
from test_gpu_frame import _render_frame
from yolo_ppf_pose_estimation_amd import _capi, synth
from yolo_ppf_pose_estimation_amd._capi import FrameDetection, IcpParams, MatchFrameStats, Pose, check, lib
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEFAULTS = dict(leaf=0.003, mean_k=50, stddev_mul=1.0, normal_k=30, curvature_threshold=0.03)


def icp_params(flags=0):
    p = IcpParams()
    lib().ppf_default_icp_params(C.byref(p))
    p.flags = flags
    return p


def per_detection(det, model_cloud, obj, edge, mp, ip, top):
    """the per-detection route: (rows as bytes, ICP iterations)"""
    if det is None or len(obj) == 0 or (edge is not None and len(edge) == 0):
        return [], []
    cap = len(obj) + 8
    out, n = (Pose * cap)(), C.c_int(0)
    check(lib().ppf_match_clouds(det._model.ptr, obj._ptr, edge._ptr if edge is not None else None, C.byref(mp), out, cap, C.byref(n)))
    k = min(top, n.value)
    if k == 0:
        return [], []
    it = (C.c_int * k)()
    check(lib().ppf_icp_refine_clouds(model_cloud._ptr, obj._ptr, C.byref(ip), out, k, it))
    return [bytes(out[i]) for i in range(k)], list(it)


def match_frame(entries, mp, ip, top):
    """entries: (detector or None, model cloud, object cloud, edge cloud or None) -> (rows per detection, iterations, stats)"""
    n = len(entries)
    dets = (FrameDetection * max(n, 1))()
    for i, (det, mc, obj, edge) in enumerate(entries):
        if det is None:
            continue
        dets[i].model, dets[i].model_cloud, dets[i].scene = det._model.ptr, mc._ptr, obj._ptr
        dets[i].edge = edge._ptr if edge is not None else None
    out = (Pose * (max(n, 1) * top))()
    n_out = (C.c_int * max(n, 1))()
    it = (C.c_int32 * (max(n, 1) * top))()
    st = MatchFrameStats()
    check(lib().ppf_match_frame(dets, n, C.byref(mp), C.byref(ip), top, out, n_out, it, C.byref(st)))
    rows = [[bytes(out[i * top + k]) for k in range(n_out[i])] for i in range(n)]
    iters = [[it[i * top + k] for k in range(n_out[i])] for i in range(n)]
    return rows, iters, st


def check_against_loop(entries, mp, ip, top):
    rows, iters, st = match_frame(entries, mp, ip, top)
    for i, (det, mc, obj, edge) in enumerate(entries):
        want_rows, want_it = per_detection(det, mc, obj, edge, mp, ip, top)
        assert rows[i] == want_rows, i
        assert iters[i] == want_it, i
    assert st.n_icp_jobs == sum(len(r) for r in rows)
    assert st.n_matched == sum(1 for r in rows if r)
    return rows, iters, st


@pytest.fixture(scope="module")
def c1(bottle):
    xyz, depth, box, intr = D.c1_frame()
    scene = DeviceCloud.upload(xyz)
    pairs = scene.prep_frame([box, (5, 5, 10, 10)], depth, intr, DEFAULTS)   # the second box lies where the depth image is empty
    det = PPF3DDetector(0.025, 0.05).trainModel(bottle)
    return det, DeviceCloud.upload(bottle), pairs[0][0], pairs[0][1], det._params(0.05, 0.05, False), pairs[1]


def test_c1_frame_reproduces_the_golden_result(c1):
    golden = np.load(os.path.join(GOLDEN, "c1_pipeline_golden.npz"))
    det, mc, obj, edge = c1[:4]
    mp = c1[4]
    cap = len(obj) + 8
    matched, n = (Pose * cap)(), C.c_int(0)
    check(lib().ppf_match_clouds(det._model.ptr, obj._ptr, edge._ptr, C.byref(mp), matched, cap, C.byref(n)))
    rows, iters, st = check_against_loop([(det, mc, obj, edge)], mp, icp_params(), 5)
    poses = [Pose.from_buffer_copy(r) for r in rows[0]]
    assert [p.num_votes for p in poses] == golden["top_votes"].tolist()
    assert iters[0] == golden["icp_iterations"].tolist()
    # the ICP starts from the device's own match poses: where those are the golden ones bit for bit, so is the result
    same_start = all(np.array_equal(np.array(matched[i].pose).reshape(4, 4), golden["match_poses"][i]) for i in range(5))
    for i, p in enumerate(poses):
        if same_start:
            np.testing.assert_array_equal(np.array(p.pose).reshape(4, 4), golden["icp_poses"][i])
            assert p.residual == golden["icp_residuals"][i]
        else:
            np.testing.assert_allclose(np.array(p.pose).reshape(4, 4), golden["icp_poses"][i], rtol=0, atol=1e-9)
    assert (st.n_dets, st.n_matched, st.n_icp_jobs) == (1, 1, 5)


def test_duplicates_share_one_launch_sequence(c1):
    det, mc, obj, edge, mp, _ = c1
    ip = icp_params()
    base, base_it, st1 = match_frame([(det, mc, obj, edge)], mp, ip, 5)
    assert len(base[0]) == 5
    for K in (3, 8, 16):
        rows, iters, st = match_frame([(det, mc, obj, edge)] * K, mp, ip, 5)
        assert rows == base * K and iters == base_it * K, K
        assert st.n_icp_jobs == 5 * K
        if K == 16:
            assert st.n_icp_launches <= st1.n_icp_launches + 4 * ip.num_levels, (st.n_icp_launches, st1.n_icp_launches)
            assert st.n_icp_launches < 16 * st1.n_icp_launches / 4


def test_more_poses_than_one_launch_sequence(c1):
    """20 detections x top 16: more ICP jobs than one launch sequence holds (256), so two sequences run"""
    det, mc, obj, edge, mp, _ = c1
    ip = icp_params()
    base, base_it, _ = match_frame([(det, mc, obj, edge)], mp, ip, 16)
    assert len(base[0]) == 16
    rows, iters, st = match_frame([(det, mc, obj, edge)] * 20, mp, ip, 16)
    assert st.n_icp_jobs == 320
    assert rows == base * 20 and iters == base_it * 20


@pytest.fixture(scope="module")
def rendered(bottle):
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    p = dict(DEFAULTS, leaf=0.004)
    pairs = DeviceCloud.upload(scene).prep_frame(boxes, depth, intr, p)
    det_b = PPF3DDetector(0.05, 0.05).trainModel(bottle)
    det_s = PPF3DDetector(0.05, 0.05).trainModel(solid)
    return pairs, (det_b, DeviceCloud.upload(bottle)), (det_s, DeviceCloud.upload(solid)), det_b._params(0.05, 0.05, False)


def test_mixed_models_none_and_empty_detections(rendered, c1):
    pairs, (db, cb), (ds, cs), mp = rendered
    empty = c1[5]
    assert len(empty[0]) == 0
    entries = [(db, cb, pairs[0][0], pairs[0][1]), (None, None, pairs[1][0], pairs[1][1]), (ds, cs, pairs[2][0], pairs[2][1]),
               (db, cb, empty[0], empty[1]), (db, cb, pairs[1][0], pairs[1][1]), (ds, cs, pairs[0][0], pairs[0][1]),
               (c1[0], c1[1], c1[2], c1[3])]
    rows, iters, st = check_against_loop(entries, mp, icp_params(), 5)
    assert rows[1] == [] and rows[3] == []
    assert rows[0] and rows[2] and rows[4]
    assert st.n_dets == 7


@pytest.fixture(scope="module")
def synthetic():
    models = []
    for kind, n, seed in (("box", 3000, 1), ("cylinder", 6000, 2), ("torus", 1500, 3), ("box", 12000, 4)):
        m = synth.make_solid(kind, n, seed=seed)
        models.append((PPF3DDetector(0.05, 0.05).trainModel(m), DeviceCloud.upload(m), m))
    return models


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_sweep_every_detection_equals_the_loop(synthetic, seed):
    rng = np.random.default_rng(100 + seed)
    mp = synthetic[0][0]._params(0.05, 0.05, False)
    ip = icp_params()
    draws = [(int(rng.integers(1, 13)), int(rng.choice([1, 5, 8, 16]))) for _ in range(2)]
    draws.append((12, 8) if seed == 0 else (9, 16))              # > 8 and > 64 poses in one call
    for K, top in draws:
        entries = []
        for _ in range(K):
            det, mc, m = synthetic[int(rng.integers(0, len(synthetic)))]
            scene, _ = synth.make_scene(m, n_points=int(rng.integers(800, 4000)), seed=int(rng.integers(1 << 30)))
            obj = DeviceCloud.upload(np.ascontiguousarray(scene, np.float32))
            edge = DeviceCloud.upload(np.ascontiguousarray(scene[::3], np.float32)) if rng.random() < 0.5 else None
            entries.append((det, mc, obj, edge))
        rows, _, st = check_against_loop(entries, mp, ip, top)
        assert st.n_dets == K


def test_flags_give_the_same_rows(c1, rendered):
    det, mc, obj, edge, mp, _ = c1
    pairs, (db, cb), (ds, cs), _ = rendered
    entries = [(det, mc, obj, edge), (ds, cs, pairs[2][0], pairs[2][1]), (det, mc, obj, edge)]
    ref = match_frame(entries, mp, icp_params(), 5)
    for flags in (_capi.PPF_ICP_GRID_ALWAYS, _capi.PPF_ICP_LEGACY):
        got = match_frame(entries, mp, icp_params(flags), 5)
        assert got[0] == ref[0] and got[1] == ref[1], flags


def test_two_concurrent_callers(c1, rendered):
    det, mc, obj, edge, mp, _ = c1
    pairs, (db, cb), (ds, cs), _ = rendered
    a = [(det, mc, obj, edge)] * 4
    b = [(db, cb, pairs[0][0], pairs[0][1]), (ds, cs, pairs[2][0], pairs[2][1])] * 3
    ip = icp_params()
    want = [match_frame(a, mp, ip, 5)[:2], match_frame(b, mp, ip, 5)[:2]]
    got = [None, None]
    errs = []
    start = threading.Barrier(2)

    def run(k, entries):
        try:
            start.wait()
            for _ in range(3):   # one of the two holds the pooled ICP scratch, the other works on a private one
                r = match_frame(entries, mp, ip, 5)[:2]
                if r != want[k]:
                    got[k] = r
                    return
            got[k] = want[k]
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(0, a)), threading.Thread(target=run, args=(1, b))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert got[0] == want[0] and got[1] == want[1]


def test_match_frame_wrapper_equals_the_loop(bottle):
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    cp = CloudProcessor(scene, depth, boxes, [39, 39, 73], [0, 1, 2], 0.05, 0.05)
    cp.LoadSingleModel(bottle, "bottle")
    cp.LoadSingleModel(solid, "box")
    cp.TrainDetector(0.05, 0.05)
    cp.PrepareFrame(K, 0.004, 50, 1.0, 30, 0.03)
    for labels in (["bottle", "bottle", "box"], ["box", None, "bottle"], [None, None, None]):
        one = cp.MatchFrame(labels)
        assert "match_frame" in cp.timings
        loop = cp.MatchFrame(labels, one_pass=False)
        assert len(one) == len(loop) == 3
        for p, q in zip(one, loop):
            assert (p is None) == (q is None)
            if p is not None:
                np.testing.assert_array_equal(p.pose, q.pose)
                assert (p.numVotes, p.residual, p.angle) == (q.numVotes, q.residual, q.angle)
                np.testing.assert_array_equal(p.q, q.q)
                np.testing.assert_array_equal(p.t, q.t)


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_cpp_facade_match_frame(tmp_path, bottle, compiler):
    xyz, depth, box, intr = D.c1_frame()
    x, y, w, h = box
    boxes = np.asarray([box, (x - 10, y - 15, w + 30, h + 25), box], np.int32)
    exe = str(tmp_path / "frame_match_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frame_match_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}",
                    "-o", exe], check=True)
    (tmp_path / "scene.f32").write_bytes(np.ascontiguousarray(xyz, np.float32).tobytes())
    (tmp_path / "depth.f32").write_bytes(np.ascontiguousarray(depth, np.float32).tobytes())
    (tmp_path / "boxes.i32").write_bytes(boxes.tobytes())
    (tmp_path / "model.f32").write_bytes(np.ascontiguousarray(bottle, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "scene.f32"), str(xyz.shape[0]), str(tmp_path / "depth.f32"), str(depth.shape[0]),
                        str(depth.shape[1])] + [repr(float(v)) for v in intr] +
                       [str(tmp_path / "boxes.i32"), str(len(boxes)), str(tmp_path / "model.f32"), str(bottle.shape[0])],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    Kmat = np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1.0]])
    cp = CloudProcessor(xyz, depth, [tuple(int(v) for v in b) for b in boxes], [39] * 3, [0] * 3, 0.025, 0.05)
    cp.LoadSingleModel(bottle, "bottle")
    cp.TrainDetector(0.025, 0.05)
    cp.PrepareFrame(Kmat, 0.003, 50, 1.0, 30, 0.03)
    poses = cp.MatchFrame(["bottle"] * 3)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4
    for i, p in enumerate(poses):
        f = lines[i].split()
        assert f[0] == "det" and p is not None, lines[i]
        assert int(f[5]) == p.numVotes and float(f[9]) == p.residual
        np.testing.assert_array_equal(np.array([float(v) for v in f[11:27]]).reshape(4, 4), p.pose)
    f = lines[-1].split()   # launches and syncs may differ by a pass per level between two runs (passes launched ahead)
    assert f[0] == "icp_jobs" and int(f[1]) == cp.match_frame_stats["n_icp_jobs"] == 15 and int(f[3]) > 0
