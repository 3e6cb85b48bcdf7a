"""ppf_refine_frame on the device against the numpy restatement of DESIGN.md §17 (tests/refine_oracle.py): the refined
matrices and every info field byte for byte over models of 50, 128 and 3,001 rows, both model steps and every status; a job's
bytes do not depend on the rest of the call; the in-place call; max_iters 0; constant launch and read-back counts; and the
chain prep -> match -> select -> refine on the two-bottle frame, then the same poses tracked into a second frame; the edge
cases of tests/refine_cases.py (image borders, depth holes, non-finite rows and poses, the guards at equality, tied pivots, the
sizes at the tiles of the sums), more jobs than compute units, and seeded random draws."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refine_cases as RC
import refine_oracle as R
import render_oracle as RO
from conftest import soak_seeds
from test_gpu_frame import LAYOUT, _render_frame
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import FrameDetection, Pose, RefineInfo, RefineParams, RefineStats, check, lib
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, refine_frame, select_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")

ROWS, COLS = 120, 160
INTR = (300.0, 300.0, 79.5, 59.5)
TOP = 4
SIZES = (50, 128, 3001)   # a chunk tail, whole chunks, more rows than a workgroup has threads


@pytest.fixture(scope="module")
def case():
    """three samplings of one ellipsoid at one true pose, the image of the densest, and four starts per model from the
    truth itself to (10 mm, 5 deg)"""
    models = [R.ellipsoid(n, seed=7 + n) for n in SIZES]
    T = np.eye(4)
    T[:3, :3] = R.rot_vec([0.4, -0.3, 0.2])
    T[:3, 3] = [0.01, -0.005, 0.6]
    zb = RO.zbuffer(R.transform_rows(models[2], T), ROWS, COLS, INTR, 0.003)
    depth = zb.view(np.float32).copy()
    depth[zb == RO.EMPTY32] = 0.9
    centre = T[:3, 3].copy()
    poses = []
    for i in range(3):
        starts = [T.copy()]
        for k, (mm, deg) in enumerate(((2, 1), (5, 3), (10, 5))):
            t, r = R.random_offset(np.random.default_rng(100 * i + k), mm, deg)
            starts.append(R.offset_pose(T, centre, t, r))
        poses.append(starts)
    far = T.copy()
    far[0, 3] += 0.2   # off the object: no pairs
    poses[1][3] = far
    return dict(models=models, clouds=[DeviceCloud.upload(m) for m in models], T=T, depth=depth, poses=poses)


def call(clouds, poses, depth, intr, prm=None, top=TOP, in_place=False, with_info=True):
    """ppf_refine_frame through ctypes: (matrices (n, top, 4, 4), info rows (n, top), stats, the out records)"""
    n = len(clouds)
    dets = (FrameDetection * max(n, 1))()
    recs = (Pose * (max(n, 1) * top))()
    n_poses = (C.c_int * max(n, 1))()
    for i, (c, plist) in enumerate(zip(clouds, poses)):
        dets[i].model_cloud = c._ptr
        n_poses[i] = len(plist)
        for k, T in enumerate(plist):
            recs[i * top + k].pose[:] = np.asarray(T, dtype=np.float64).reshape(16).tolist()
            recs[i * top + k].num_votes, recs[i * top + k].alpha = 10 * i + k, 0.25 * k
    p = RefineParams()
    lib().ppf_default_refine_params(C.byref(p))
    for key, v in (prm or {}).items():
        setattr(p, key, v)
    out = recs if in_place else (Pose * (max(n, 1) * top))()
    info = (RefineInfo * (max(n, 1) * top))()
    st = RefineStats()
    img = np.ascontiguousarray(depth, dtype=np.float32)
    check(lib().ppf_refine_frame(dets, n, recs, n_poses, top, img.ctypes.data, img.shape[0], img.shape[1], (C.c_double * 4)(*intr),
                                 C.byref(p), out, info if with_info else None, C.byref(st)))
    mats = np.array([list(out[j].pose) for j in range(n * top)], dtype=np.float64).reshape(n, top, 4, 4)
    return mats, np.ctypeslib.as_array(info).copy()[:n * top].reshape(n, top), _capi.stats_dict(st), out


def assert_job(mat, info, want_T, want_info, what):
    for f in R.INFO_FIELDS:
        a = np.asarray(info[f])
        b = np.asarray(want_info[f], dtype=a.dtype)
        assert a.tobytes() == b.tobytes(), (what, f, info[f], want_info[f])
    assert mat.tobytes() == np.asarray(want_T, dtype=np.float64).tobytes(), (what, mat, want_T)


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
def test_byte_parity_with_the_oracle(case):
    seen = set()
    n_poses = [3, 4, 4]
    poses = [plist[:n] for plist, n in zip(case["poses"], n_poses)]
    for prm in (dict(model_step=1), dict(model_step=3), dict(model_step=1, max_iters=2), dict(model_step=1, max_step_trans=0.002)):
        mats, info, st, out = call(case["clouds"], poses, case["depth"], INTR, prm)
        assert st["n_jobs"] == 11 and st["n_launches"] == 1 and st["n_host_syncs"] == 1
        for i in range(3):
            for k in range(n_poses[i]):
                T, want = R.refine(case["models"][i], poses[i][k], case["depth"], INTR, prm)
                assert_job(mats[i, k], info[i, k], T, want, (prm, i, k))
                seen.add(int(info[i, k]["status"]))
                rec = out[i * TOP + k]
                assert (rec.num_votes, rec.alpha) == (10 * i + k, 0.25 * k)
                assert np.float64(rec.residual).tobytes() == np.float64(want["rmse_last"]).tobytes()
                if want["iterations"] > 0:
                    assert list(rec.t) == [T[0, 3], T[1, 3], T[2, 3]] and abs(np.linalg.norm(rec.q) - 1) < 1e-12
        # the row past detection 0's poses: NONE, all zero, the pose record untouched
        assert info[0, 3].tobytes() == bytes(C.sizeof(RefineInfo)) and bytes(out[3]) == bytes(Pose())
        seen.add(int(info[0, 3]["status"]))
    assert seen == {R.NONE, R.CONVERGED, R.MAX_ITERS, R.LOST, R.STEP}, seen
    # the refined poses are the true one: the (10 mm, 5 deg) start of the densest model ends within a quarter pixel
    mats, info, _, _ = call(case["clouds"], poses, case["depth"], INTR)
    assert info[2, 3]["status"] == R.CONVERGED and R.mean_row_error(case["models"][2], mats[2, 3], case["T"]) < 0.0005


# ---- 2. a job depends on nothing else ------------------------------------------------------------------------------------------
def test_a_job_alone_and_among_eleven_others(case):
    mats, info, _, _ = call(case["clouds"], case["poses"], case["depth"], INTR)
    again = call(case["clouds"], case["poses"], case["depth"], INTR)
    assert mats.tobytes() == again[0].tobytes() and info.tobytes() == again[1].tobytes()
    for i, k in ((0, 3), (1, 1), (2, 2), (1, 3)):
        m1, i1, st, _ = call([case["clouds"][i]], [[case["poses"][i][k]]], case["depth"], INTR, top=1)
        assert st["n_jobs"] == 1
        assert m1[0, 0].tobytes() == mats[i, k].tobytes() and i1[0, 0].tobytes() == info[i, k].tobytes(), (i, k)


def test_in_place_and_without_info(case):
    mats, info, _, out = call(case["clouds"], case["poses"], case["depth"], INTR)
    m2, _, _, out2 = call(case["clouds"], case["poses"], case["depth"], INTR, in_place=True, with_info=False)
    assert bytes(out) == bytes(out2) and mats.tobytes() == m2.tobytes()


def test_max_iters_zero_returns_the_input(case):
    mats, info, st, out = call(case["clouds"], case["poses"], case["depth"], INTR, dict(max_iters=0))
    assert st["n_launches"] == 0 and st["n_host_syncs"] == 0 and st["n_jobs"] == 12
    for i in range(3):
        for k in range(4):
            assert mats[i, k].tobytes() == np.asarray(case["poses"][i][k]).tobytes()
            assert (info[i, k]["status"], info[i, k]["iterations"], info[i, k]["n_rows"]) == (R.MAX_ITERS, 0, SIZES[i])
            assert out[i * TOP + k].residual == 0.0


def test_launch_counts_do_not_depend_on_the_detections(case):
    one = call([case["clouds"][2]], [case["poses"][2]], case["depth"], INTR)[2]
    eight = call([case["clouds"][i % 3] for i in range(8)], [case["poses"][i % 3] for i in range(8)], case["depth"], INTR)[2]
    assert (one["n_launches"], one["n_host_syncs"]) == (eight["n_launches"], eight["n_host_syncs"]) == (1, 1)
    assert (one["n_jobs"], eight["n_jobs"]) == (4, 32)
    none = call([case["clouds"][0]], [[]], case["depth"], INTR)[2]
    assert (none["n_launches"], none["n_host_syncs"], none["n_jobs"]) == (0, 0, 0)


# ---- 3. the chain on the device ------------------------------------------------------------------------------------------------
def mean_dist(model, Ta, Tb):
    return R.mean_row_error(model, Ta, Tb)


def render_moved(depth0, K, objs_before, objs_after):
    """frame t + 1 of _render_frame's scene: the background plane again where the objects were, the moved objects splatted as
    _render_frame splats them"""
    rows, cols = depth0.shape
    fx, fy, ppx, ppy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    vv, uu = np.mgrid[0:rows, 0:cols]
    ray = np.stack([(uu - ppx) / fx, (vv - ppy) / fy, np.ones_like(uu, dtype=np.float64)], axis=-1)
    nrm = np.array([0.1, -0.15, -1.0]) / np.linalg.norm([0.1, -0.15, -1.0])
    depth = (-0.95 / (ray @ nrm)).astype(np.float32)
    for model, T in objs_after:
        obj = model[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        pu = np.round(obj[:, 0] / obj[:, 2] * fx + ppx).astype(int)
        pv = np.round(obj[:, 1] / obj[:, 2] * fy + ppy).astype(int)
        order = np.argsort(-obj[:, 2])
        for du in (0, 1):
            for dv in (0, 1):
                depth[np.clip(pv[order] + dv, 0, rows - 1), np.clip(pu[order] + du, 0, cols - 1)] = obj[order, 2]
    return depth


def test_end_to_end_polish_and_tracking(bottle):
    """prep -> match -> select (min_score 0.3) -> refine on the two-bottle frame: both bottles stay within the 3 mm
    test_gpu_select.py asserts; then the same poses against a second frame with both bottles moved by (4 mm, 2 deg about the
    vertical) end within 3 mm of the moved truth.  The bottle is a solid of revolution: the spin about its axis is not
    observable, so the distances are taken between the models' rows, which the spin moves little, and the damping leaves
    it where it was."""
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    assert len(LAYOUT) == 3
    cp = CloudProcessor(scene, depth, boxes, [39, 39, 73], [0, 1, 2], 0.05, 0.05)
    cp.LoadSingleModel(bottle, "bottle")
    cp.TrainDetector(0.05, 0.05)
    cp.PrepareFrame(K, 0.004, 50, 1.0, 30, 0.03)
    cp.MatchFrame(["bottle", "bottle", None])
    chosen = cp.SelectFrame(min_score=0.3)
    assert sorted(i for i, _, _ in chosen) == [0, 1]
    before = {i: (P.pose.copy(), float(cp.select_info[i, k]["explained"])) for i, k, P in chosen}
    print("explained of every pose held, bottles 0 and 1:", cp.select_info["explained"][:2].tolist())
    cp.RefineFrame(selected_only=True)
    assert cp.refine_stats["n_launches"] == 1 and cp.refine_stats["n_host_syncs"] == 1 and cp.refine_stats["n_jobs"] == 2
    assert "refine_frame" in cp.timings
    for i, k, _ in chosen:
        row = cp.refine_info[i, 0]
        assert row["status"] in (R.CONVERGED, R.MAX_ITERS) and row["iterations"] > 0, row
        d0, d1 = mean_dist(bottle, before[i][0], objs[i][1]), mean_dist(bottle, cp.frame_poses[i][k].pose, objs[i][1])
        print(f"bottle {i}: {d0 * 1e3:.2f} mm -> {d1 * 1e3:.2f} mm from the truth, {int(row['iterations'])} iterations, rmse "
              f"{float(row['rmse_first']) * 1e3:.2f} -> {float(row['rmse_last']) * 1e3:.2f} mm")
        assert d1 <= 0.003, (i, d0, d1)
        # the wrapper's result is the oracle's
        T, want = R.refine(bottle, before[i][0], depth, cp.frame_intr)
        assert cp.frame_poses[i][k].pose.tobytes() == T.tobytes() and int(row["status"]) == want["status"]
    # select again on the two polished poses alone: a re-selection among all of a detection's poses may as well take an
    # unrefined sibling of the polished one (they lie within a pixel of each other; on the device it took k 3 and 2), so
    # which k wins there is no property of the refinement.  Poses within 3 mm of the truth pass the 0.3 gate and the two
    # bottles do not overlap: both are selected again.
    polished = [[], [], []]
    for i, k, _ in chosen:
        polished[i] = [cp.frame_poses[i][k]]
    info, sel = select_frame([cp._model_clouds[0] if p else None for p in polished], polished, depth, cp.frame_intr, dict(min_score=0.3))
    assert sorted(sel.tolist()) == [0, 1], (sel, info)
    for i in sorted(before):
        print(f"bottle {i}: explained {before[i][1]:.4f} -> {float(info[i, 0]['explained']):.4f}")
    # frame t + 1
    moved = []
    for model, T in objs[:2]:
        c = T[:3, :3] @ model[:, :3].astype(np.float64).mean(axis=0) + T[:3, 3]
        moved.append((model, R.offset_pose(T, c, [0.004, 0.0, 0.0], [0.0, np.radians(2.0), 0.0])))
    depth2 = render_moved(depth, K, objs, moved + [objs[2]])
    held = {i: cp.frame_poses[i][k].pose.copy() for i, k, _ in chosen}
    cp.RefineFrame(depth=depth2, selected_only=True)
    for i, k, _ in chosen:
        row = cp.refine_info[i, 0]
        d0, d1 = mean_dist(bottle, held[i], moved[i][1]), mean_dist(bottle, cp.frame_poses[i][k].pose, moved[i][1])
        print(f"bottle {i} tracked: {d0 * 1e3:.2f} mm -> {d1 * 1e3:.2f} mm from the moved truth, status {int(row['status'])}, "
              f"{int(row['iterations'])} iterations")
        assert row["status"] in (R.CONVERGED, R.MAX_ITERS) and d1 <= 0.003, (i, d0, d1, row)
    # the free function, and its errors
    refined, info = refine_frame([cp._model_clouds[0]], [[held[0]]], depth2, cp.frame_intr)
    k0 = [k for i, k, _ in chosen if i == 0][0]
    assert refined[0][0].pose.tobytes() == cp.frame_poses[0][k0].pose.tobytes() and info[0, 0].tobytes() == cp.refine_info[0, 0].tobytes()
    with pytest.raises(_capi.PPFError):
        refine_frame([cp._model_clouds[0]], [[held[0]]], None, cp.frame_intr)
    with pytest.raises(_capi.PPFError):
        refine_frame([cp._model_clouds[0]], [[held[0]]], depth2, cp.frame_intr, dict(min_pairs=2))


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_cpp_facade_refine_frame(tmp_path, bottle, compiler):
    """examples/frame_refine_demo.cpp (prepareFrame -> matchFrame -> selectFrame -> refineFrame, polish then tracking) prints
    what the Python chain computes"""
    from test_gpu_select import RP, UNION, device_poses
    from test_gpu_verify import DEFAULTS
    scene, depth, boxes, K, objs, _ = _render_frame(bottle)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    moved = []
    for model, T in objs[:2]:
        c = T[:3, :3] @ model[:, :3].astype(np.float64).mean(axis=0) + T[:3, 3]
        moved.append((model, R.offset_pose(T, c, [0.004, 0.0, 0.0], [0.0, np.radians(2.0), 0.0])))
    depth2 = render_moved(depth, K, objs, moved + [objs[2]])
    exe = str(tmp_path / "frame_refine_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frame_refine_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}",
                    "-o", exe], check=True)
    b = np.asarray([boxes[0], boxes[1], UNION], np.int32)
    for name, a in (("scene.f32", np.ascontiguousarray(scene, np.float32)), ("depth.f32", np.ascontiguousarray(depth, np.float32)),
                    ("next.f32", depth2), ("boxes.i32", b), ("model.f32", np.ascontiguousarray(bottle, np.float32))):
        (tmp_path / name).write_bytes(a.tobytes())
    r = subprocess.run([exe, str(tmp_path / "scene.f32"), str(scene.shape[0]), str(tmp_path / "depth.f32"), str(depth.shape[0]),
                        str(depth.shape[1])] + [repr(float(v)) for v in intr] +
                       [str(tmp_path / "boxes.i32"), str(len(b)), str(tmp_path / "model.f32"), str(bottle.shape[0]), "0.3",
                        str(tmp_path / "next.f32")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the demo's chain from Python: prepareFrame's default stages (leaf 3 mm), matchFrame with top 8
    mcloud = DeviceCloud.upload(bottle)
    pairs = DeviceCloud.upload(scene).prep_frame([tuple(v) for v in b.tolist()], depth, intr, DEFAULTS)
    poses = device_poses(dict(pairs=pairs, mcloud=mcloud), bottle)
    top = max(len(p) for p in poses)
    _, sel = select_frame([mcloud] * 3, poses, depth, intr, dict(min_score=0.3), RP)
    held = [[poses[j // top][j % top]] for j in sel.tolist()]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 * len(sel) + 1 and len(sel) == 2, r.stdout
    at = 0
    for what, img in (("polish", depth), ("track", depth2)):
        refined, info = refine_frame([mcloud] * len(held), held, img, intr)
        for rnk, j in enumerate(sel.tolist()):
            f = lines[at].split()
            at += 1
            assert f[:5] == [what, "det", str(j // top), "k", f"{j % top}:"], lines[at - 1]
            for name, v in zip(R.INFO_FIELDS, f[6:22:2]):
                if name.startswith("rmse"):
                    assert np.float32(float(v)).tobytes() == np.float32(info[rnk, 0][name]).tobytes(), (what, rnk, name)
                else:
                    assert int(v) == int(info[rnk, 0][name]), (what, rnk, name)
            assert f[5:21:2] == R.INFO_FIELDS and f[21] == "pose"
            assert np.array([float(v) for v in f[22:38]]).tobytes() == refined[rnk][0].pose.tobytes(), (what, rnk)
        if what == "polish":
            assert lines[at] == f"jobs {len(sel)} launches 1 read-backs 1"
            at += 1
        held = [[refined[rnk][0]] for rnk in range(len(sel))]


# ---- 4. the edges: tests/refine_cases.py on the device --------------------------------------------------------------------------
def assert_run(r, what):
    """one call for the run r of refine_cases.py: every pose's matrix, info row and residual are the oracle's bytes, a pose no
    step was applied to keeps its record, the hand counts hold on the device's info, rows without a pose stay NONE.  Returns
    the statuses seen."""
    clouds = [DeviceCloud.upload(m) for m in r["models"]]
    top = max(len(plist) for plist in r["poses"])
    mats, info, st, out = call(clouds, r["poses"], r["depth"], r["intr"], r["prm"], top=top)
    assert (st["n_jobs"], st["n_launches"], st["n_host_syncs"]) == (sum(len(plist) for plist in r["poses"]), 1, 1), (what, st)
    seen = set()
    for i, plist in enumerate(r["poses"]):
        for k, T0 in enumerate(plist):
            T, want = R.refine(r["models"][i], T0, r["depth"], r["intr"], r["prm"])
            assert_job(mats[i, k], info[i, k], T, want, (what, i, k))
            for f, v in r["hand"].get((i, k), {}).items():
                assert int(info[i, k][f]) == v, (what, i, k, f, info[i, k])
            rec = out[i * top + k]
            assert np.float64(rec.residual).tobytes() == np.float64(want["rmse_last"]).tobytes(), (what, i, k)
            if want["iterations"] == 0:   # the record as given, apart from the residual
                given = Pose()
                given.pose[:] = np.asarray(T0, dtype=np.float64).reshape(16).tolist()
                given.num_votes, given.alpha, given.residual = 10 * i + k, 0.25 * k, rec.residual
                assert bytes(rec) == bytes(given), (what, i, k)
            seen.add(int(info[i, k]["status"]))
        for k in range(len(plist), top):
            assert info[i, k].tobytes() == bytes(C.sizeof(RefineInfo)) and bytes(out[i * top + k]) == bytes(Pose()), (what, i, k)
            seen.add(int(info[i, k]["status"]))
    return seen


_SEEN = {}


@pytest.mark.parametrize("name", RC.NAMES)
def test_byte_parity_on_the_edge_cases(name):
    c = RC.case(name)
    _SEEN[name] = set()
    for r in c["runs"]:
        _SEEN[name] |= assert_run(r, (name, r["what"]))
    if name == RC.NAMES[-1] and len(_SEEN) == len(RC.NAMES):   # the whole set ran: every status without the old fixture
        assert set().union(*_SEEN.values()) == {R.NONE, R.CONVERGED, R.MAX_ITERS, R.LOST, R.STEP}, _SEEN


def test_more_jobs_than_compute_units(case):
    """24 detections x 16 poses, 384 workgroups on 256 CUs: each job's bytes are those of the same (model, pose) alone"""
    aside = np.eye(4)
    aside[:3, 3] = [0.2, 0.1, -0.1]   # the plane on the background at 0.9, beside the object
    plane = RC.plane64()
    models = [case["models"][0], case["models"][1], plane]
    clouds = [case["clouds"][0], case["clouds"][1], DeviceCloud.upload(plane)]
    starts = [case["poses"][0], case["poses"][1],
              [aside, R.offset_pose(aside, np.array([0.2, 0.1, 0.9]), [0.0, 0.0, 0.002], [0.0, 0.0, 0.0]),
               R.offset_pose(aside, np.array([0.2, 0.1, 0.9]), [0.001, 0.001, 0.002], [0.01, -0.005, 0.02])]]
    alone = {}
    for m in range(3):
        for s, T0 in enumerate(starts[m]):
            m1, i1, st, _ = call([clouds[m]], [[T0]], case["depth"], INTR, top=1)
            alone[m, s] = (m1[0, 0].tobytes(), i1[0, 0].tobytes())
            T, want = R.refine(models[m], T0, case["depth"], INTR)
            assert_job(m1[0, 0], i1[0, 0], T, want, ("alone", m, s))
    which = [[(d % 3, (d // 3 + k) % len(starts[d % 3])) for k in range(16)] for d in range(24)]
    mats, info, st, _ = call([clouds[m] for m, _ in (w[0] for w in which)], [[starts[m][s] for m, s in w] for w in which], case["depth"], INTR, top=16)
    assert (st["n_jobs"], st["n_launches"], st["n_host_syncs"]) == (384, 1, 1), st
    assert {int(v) for v in info["status"].ravel()} >= {R.CONVERGED, R.LOST}
    for d, w in enumerate(which):
        for k, (m, s) in enumerate(w):
            assert (mats[d, k].tobytes(), info[d, k].tobytes()) == alone[m, s], (d, k, m, s)


@pytest.mark.parametrize("seed", soak_seeds(6, "PPF_SOAK_REFINE"))
def test_refine_random_draw(seed):
    cfg, r = RC.random_draw(seed)
    assert_run(r, cfg)
