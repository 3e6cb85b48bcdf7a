"""ppf_depth_motion on the device against tests/depth_motion_oracle.py, byte for byte: the pose, every level row and the
counts, at the smallest shapes that reach each path of the kernels (less than one chunk, odd sizes, a partial last group, the
third tree level), for both formats and entries, pitched and misaligned rows, spoiled pixels, every status, determinism, the
refusals of the device entry, and the wrappers: DepthOdometry, CloudProcessor.TrackCamera and the C++ demo."""
import ctypes as C
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import depth_motion_cases as Cs
import depth_motion_oracle as O
import refine_cases
import refine_oracle as R
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import lib
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DepthOdometry, DeviceCloud, _mat44_mul, depth_motion
from yolo_ppf_pose_estimation_amd.detector import Pose3D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
F32 = np.float32
FAILED = (O.LOST, O.STEP)


def device(prev, cur, intr, p=None, init=None, **kw):
    return depth_motion(prev, cur, intr, params=p, init=init, return_info=True, return_stats=True, **kw)


def same(got, want, what=""):
    """the device's (T, rows, stats) against the oracle's: bytes, every row field, the counts"""
    T, info, st = got
    Tw, rows, stw = want
    for l in range(O.MAX_LEVELS):
        for f in O.ROW_FIELDS:
            assert np.asarray(info[l][f]).tobytes() == np.asarray(rows[l][f], dtype=info.dtype[f]).tobytes(), (what, l, f, info[l], rows[l])
        assert not info[l]["reserved"].any()
    assert np.asarray(T).tobytes() == Tw.tobytes(), (what, T, Tw)
    for k in ("status", "n_evaluations", "n_enqueued", "n_launches", "n_host_syncs"):
        assert st[k] == stw[k], (what, k, st, stw)
    assert st["n_host_syncs"] == 1 and st["ms_wall"] > 0


def check(prev, cur, intr, p=None, init=None, what="", **kw):
    want = O.motion(prev, cur, intr, p, init, **kw)
    got = device(prev, cur, intr, p, init, **kw)
    same(got, want, what)
    return got, want


@functools.lru_cache(maxsize=None)
def sized(rows, cols, seed=1, mm=20, deg=2):
    """a noisy pair of the analytic scene at rows x cols, its intrinsics and the oracle's answer with the defaults"""
    prev, cur, T = Cs.pair(seed, mm, deg, rows=rows, cols=cols)
    intr = Cs.intrinsics(rows, cols)
    return prev, cur, intr, T, O.motion(prev, cur, intr)


# ---- the shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(24, 40), (25, 41), (66, 130)])
def test_small_shapes(rows, cols):
    """24 x 40: the coarsest level is 6 x 10 = 60 pixels, less than a chunk; 25 x 41: the odd row and column are dropped at both
    reductions; 66 x 130: 8,580 pixels = 135 chunks, three groups, the last one partial"""
    prev, cur, intr, _, want = sized(rows, cols)
    got = device(prev, cur, intr)
    same(got, want)
    assert [(r["rows"], r["cols"]) for r in want[1][:3]] == [(rows >> l, cols >> l) for l in range(3)]


@pytest.mark.parametrize("rows,cols", [(24, 40), (25, 41)])
def test_coarse_level_below_one_chunk_runs(rows, cols):
    """at the defaults the 6 x 10 level of the two small shapes has two sources and is skipped (a pixel covers 75 mm there); on
    exact images of a 5 mm / 0.5 degree motion, with gates sized to that pixel and min_pairs 6, its 60 pixels -- one partial
    chunk -- are evaluated"""
    prev, cur, _ = Cs.pair(1, 5, 0.5, rows=rows, cols=cols, noise=0.0, drop=0.0)
    got, want = check(prev, cur, Cs.intrinsics(rows, cols), dict(min_pairs=6, min_pair_share=0.0, normal_gate=0.06, pyr_gate=0.1, dist_gate=0.2))
    coarse = want[1][2]
    assert (coarse["rows"], coarse["cols"]) == (6, 10) and coarse["n_source"] >= 6 and coarse["status"] == O.CONVERGED and coarse["n_pairs_first"] >= 6


def test_third_tree_level_at_520_x_520():
    """270,400 pixels = 4,225 chunks -> 67 groups -> 2 -> 1: the only large case, run once"""
    prev, cur, intr, T_true, want = sized(520, 520)
    got = device(prev, cur, intr)
    same(got, want)
    assert want[2]["status"] not in FAILED
    assert O.group_stages((520 * 520 + 63) // 64) == 1 and (4225 + 63) // 64 == 67
    print("520 x 520: %.4f mm %.5f deg from the truth" % O.pose_error(got[0], T_true))


# ---- formats, pitches, entries -------------------------------------------------------------------------------------------
def test_uint16_images():
    prev, cur, intr, _, _ = sized(66, 130)
    a, b = Cs.to_u16(prev), Cs.to_u16(cur)
    check(a, b, intr, depth_scale=0.001)
    check(a, b, intr, depth_scale=0.0011, z_min=0.5, z_max=1.05, what="another scale and a z range")


def test_z_range_on_float_images():
    prev, cur, intr, _, _ = sized(66, 130)
    got, want = check(prev, cur, intr, z_min=0.6, z_max=0.98)
    assert want[1][0]["n_source"] < sized(66, 130)[4][1][0]["n_source"]


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_pitched_and_misaligned_rows_equal_packed_ones(u16):
    prev, cur, intr, _, want = sized(66, 130)
    kw = {}
    if u16:
        prev, cur, kw = Cs.to_u16(prev), Cs.to_u16(cur), dict(depth_scale=0.001)
        want = O.motion(prev, cur, intr, **kw)
    for pad_a, off_a, pad_b, off_b in [(3, 1, 0, 0), (0, 0, 5, 3), (2, 0, 6, 1), (6 if u16 else 2, 0, 2 if u16 else 6, 0)]:
        a, b = Cs.pitched(prev, pad_a, off_a), Cs.pitched(cur, pad_b, off_b)
        assert a.strides[0] == (130 + pad_a) * a.itemsize
        same(device(a, b, intr, **kw), want, (pad_a, off_a, pad_b, off_b))


def test_device_entry_on_a_side_stream():
    torch = pytest.importorskip("torch")
    prev, cur, intr, _, want = sized(66, 130)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        a, b = torch.from_numpy(np.array(prev)).cuda(), torch.from_numpy(np.array(cur)).cuda()
        same(device(a, b, intr), want, "packed tensors")
        # rows at a stride, starting off a 16-byte boundary
        big = torch.zeros((66, 137), dtype=torch.float32, device="cuda")
        va = big[:, 1:131]
        va.copy_(a)
        same(device(va, b, intr), want, "a strided, misaligned tensor")
    stream.synchronize()
    a16, b16 = torch.from_numpy(Cs.to_u16(prev).view(np.int16)).cuda().view(torch.uint16), torch.from_numpy(Cs.to_u16(cur).view(np.int16)).cuda().view(torch.uint16)
    same(device(a16, b16, intr), O.motion(Cs.to_u16(prev), Cs.to_u16(cur), intr), "uint16 tensors on the default stream")


def test_a_start_is_used():
    prev, cur, intr, T_true, _ = sized(66, 130)
    init = Cs.true_motion(5, 8, 1)
    got, want = check(prev, cur, intr, init=init)
    assert want[2]["status"] not in FAILED
    exact = T_true.copy()
    check(prev, cur, intr, init=exact, what="the truth as the start")


# ---- content ---------------------------------------------------------------------------------------------------------------
def test_spoiled_pixels():
    prev, cur, intr, _, _ = sized(66, 130)
    a, b = Cs.spoiled(prev, 1), Cs.spoiled(cur, 2)
    assert np.isnan(a).any() and np.isinf(a).any() and (a < 0).any() and (a == 0).any()
    got, want = check(a, b, intr)
    assert want[2]["status"] not in FAILED


def test_every_status():
    prev, cur, intr, _, want = sized(66, 130)
    # CONVERGED: identical images give the identity, byte for byte, every level converged after one evaluation
    got, same_img = check(prev, prev, intr)
    assert got[0].tobytes() == np.eye(4).tobytes()
    assert [int(r["status"]) for r in got[1][:3]] == [O.CONVERGED] * 3 and [int(r["iterations"]) for r in got[1][:3]] == [1, 1, 1]
    assert got[2]["n_evaluations"] == 3 and got[2]["n_enqueued"] == 19   # 16 evaluations returned at the state word
    # SKIPPED: nothing to see, and a level without iterations
    zero = np.zeros((66, 130), F32)
    init = Cs.true_motion(3, 10, 1)
    got, _ = check(zero, zero, intr, init=init)
    assert got[0].tobytes() == init.tobytes() and [int(r["status"]) for r in got[1]] == [O.SKIPPED] * 3 + [O.NONE]
    got, _ = check(prev, cur, intr, dict(iters=(6, 0, 3, 0)))
    assert int(got[1][1]["status"]) == O.SKIPPED and int(got[1][1]["n_source"]) > 0
    got, _ = check(prev, cur, intr, dict(iters=(0, 0, 0, 0)))
    assert got[0].tobytes() == np.eye(4).tobytes() and got[2]["n_launches"] == 6 + 3
    # LOST: a start 100 mm / 10 degrees off comes back as given
    far = Cs.true_motion(11, 100, 10)
    got, _ = check(prev, prev, intr, init=far)
    assert got[2]["status"] == O.LOST and got[0].tobytes() == far.tobytes() and int(got[1][0]["status"]) == O.NONE
    # STEP: a first step over max_step_trans
    got, _ = check(prev, cur, intr, dict(max_step_trans=0.001))
    assert got[2]["status"] == O.STEP and got[0].tobytes() == np.eye(4).tobytes() and got[2]["n_evaluations"] == 1
    # LOST at a finer level: the coarse level passes, then dist_gate leaves too few pairs
    got, wl = check(prev, cur, intr, dict(iters=(4, 0, 2, 0), min_pair_share=0.9))
    # MAX_ITERS
    got, _ = check(prev, cur, intr, dict(iters=(1, 1, 1, 1)))
    assert [int(r["status"]) for r in got[1][:3]] == [O.MAX_ITERS] * 3
    # one level, four levels
    check(prev, cur, intr, dict(levels=1, iters=(3, 0, 0, 0)))
    got, _ = check(prev, cur, intr, dict(levels=4, iters=(2, 2, 2, 2), min_pairs=6))
    assert (int(got[1][3]["rows"]), int(got[1][3]["cols"])) == (8, 16)


# ---- determinism and counts ------------------------------------------------------------------------------------------------
def test_the_same_call_twice_and_from_two_threads():
    prev, cur, intr, _, want = sized(66, 130)
    first = device(prev, cur, intr)
    second = device(prev, cur, intr)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    out = [None, None]

    def work(i):
        out[i] = [device(prev, cur, intr) for _ in range(3)]

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for runs in out:
        for got in runs:
            same(got, want)


@pytest.mark.parametrize("shape,p,launches", [((24, 40), dict(), 6 + 19 * 2), ((66, 130), dict(), 6 + 10 * 3 + 5 * 2 + 4 * 2),
                                              ((66, 130), dict(levels=2, iters=(2, 0, 0, 0)), 4 + 2 * 3 + 1)])
def test_launch_count_depends_on_sizes_and_iters_only(shape, p, launches):
    """eval + tail per evaluation, one group stage where a level has more than 64 chunks (66 x 130: 135; 33 x 65: 34)"""
    prev, cur, intr, _, _ = sized(*shape)
    for a, b in ((prev, cur), (prev, prev), (np.zeros(shape, F32), cur)):
        st = device(a, b, intr, p)[2]
        assert st["n_launches"] == launches == O.n_launches(shape, O.params(**p)) and st["n_host_syncs"] == 1


# ---- refusals of the device entry ------------------------------------------------------------------------------------------
def test_device_entry_refuses_host_memory_and_overlap():
    torch = pytest.importorskip("torch")
    prev, cur, intr, _, _ = sized(24, 40)
    it = (C.c_double * 4)(*intr)
    dp = _capi.DepthParams()
    lib().ppf_default_depth_params(C.byref(dp))
    mp = _capi.DepthMotionParams()
    lib().ppf_default_depth_motion_params(C.byref(mp))
    start = (C.c_double * 16)(*Cs.true_motion(2, 5, 1).reshape(-1))
    buf = torch.zeros(24 * 40 + 40, dtype=torch.float32, device="cuda")
    good = torch.from_numpy(np.array(cur)).cuda()

    def refused(p_prev, p_cur, text):
        pose = (C.c_double * 16)(*([7.0] * 16))
        rows = (_capi.DepthMotionLevel * 4)()
        st = _capi.DepthMotionStats()
        C.memset(rows, 0x5A, C.sizeof(rows))
        C.memset(C.byref(st), 0x5A, C.sizeof(st))
        s = lib().ppf_depth_motion_device(p_prev, 0, p_cur, 0, 24, 40, it, C.byref(dp), C.byref(mp), start, None, pose, rows, C.byref(st))
        assert s == _capi.PPF_ERR_INVALID and text in _capi.last_error(), _capi.last_error()
        assert bytes(pose) == bytes(start) and bytes(rows) == bytes(C.sizeof(rows)) and bytes(st) == bytes(C.sizeof(st))

    host = np.array(prev)
    refused(host.ctypes.data, good.data_ptr(), "(prev)")
    refused(good.data_ptr(), host.ctypes.data, "(cur)")
    refused(buf.data_ptr(), buf.data_ptr() + 40 * 4, "overlap")
    refused(buf.data_ptr(), buf.data_ptr(), "overlap")
    torch.cuda.synchronize()


# ---- the wrappers ------------------------------------------------------------------------------------------------------------
def test_depth_odometry_follows_the_oracle_chain():
    frames, poses = Cs.stream(4, seed=3, mm=15, deg=1.5, rows=66, cols=130)
    intr = Cs.intrinsics(66, 130)
    odo = DepthOdometry(66, 130, intr)
    pose = np.eye(4)
    for i, frame in enumerate(frames):
        T, status = odo.push(frame)
        if i == 0:
            assert status == _capi.PPF_MOTION_NONE and T.tobytes() == np.eye(4).tobytes()
            continue
        Tw, _, stw = O.motion(frames[i - 1], frame, intr)
        assert status == stw["status"] and status not in FAILED and T.tobytes() == Tw.tobytes()
        pose = _mat44_mul(Tw, pose)
        assert odo.pose.tobytes() == pose.tobytes() and odo.frames == i + 1
    mm, deg = O.pose_error(odo.pose, poses[-1])
    print(f"four frames of 15 mm / 1.5 degrees at 66 x 130: {mm:.3f} mm {deg:.4f} deg from the true camera pose")
    # a frame that cannot be followed leaves the pose and, unless asked, the previous frame
    held = odo.pose.copy()
    T, status = odo.push(np.zeros((66, 130), F32) + F32(0.3))   # a wall 0.3 m away: no pair within the gates
    assert status in FAILED and T.tobytes() == np.eye(4).tobytes() and odo.pose.tobytes() == held.tobytes()
    T, status = odo.push(frames[-1])
    assert status not in FAILED and odo.pose.tobytes() == _mat44_mul(T, held).tobytes()
    gpu = pytest.importorskip("torch")
    odo.reset()
    assert odo.frames == 0 and odo.pose.tobytes() == np.eye(4).tobytes()
    odo.push(gpu.from_numpy(frames[0]).cuda())
    T, status = odo.push(gpu.from_numpy(frames[1]).cuda())
    assert T.tobytes() == O.motion(frames[0], frames[1], intr)[0].tobytes()


def tracking_frames():
    """two frames of the analytic scene with an ellipsoid in front of it, the camera moved by 20 mm / 2 degrees in between:
    (frame 1, frame 2, the model, its pose in frame 1, the camera's motion)"""
    rows, cols, intr = Cs.ROWS, Cs.COLS, Cs.intrinsics()
    model = refine_cases.ellipsoid3001()
    T_obj = np.eye(4)
    T_obj[:3, :3] = R.rot_vec([0.4, -0.3, 0.2])
    T_obj[:3, 3] = [0.05, -0.02, 0.5]
    T_cam = Cs.true_motion(4, 20, 2)
    out = []
    for cam in (np.eye(4), T_cam):
        scene = Cs.render(cam).astype(F32)
        obj = refine_cases.draw(model, cam @ T_obj, 0.0, rows, cols, intr, radius=0.004)
        out.append(np.where((obj > 0) & (obj < scene), obj, scene).astype(F32))
    return out[0], out[1], model, T_obj, T_cam


def test_track_camera_then_refine_frame():
    """the pose of frame 1 carried into frame 2 by the camera's motion, then refined there: within 3 mm of the moved truth (the
    bound tests/test_gpu_refine.py holds a tracked pose to; a pixel covers 3.3 mm at the object's 0.5 m)"""
    d1, d2, model, T_obj, T_cam = tracking_frames()
    intr = Cs.intrinsics()
    cp = CloudProcessor(None, d1, [], [], [], 0.05, 0.05)
    cp.LoadSingleModel(model, "ellipsoid")
    cp._model_clouds[0] = DeviceCloud.upload(model)
    cp.frame_intr, cp.frame_labels = intr, ["ellipsoid"]
    start = Pose3D()
    start.pose = T_obj.copy()
    cp.frame_poses = [[start]]
    T, status = cp.TrackCamera(d2)
    Tw, _, stw = O.motion(d1, d2, intr)
    assert status == stw["status"] and status not in FAILED and T.tobytes() == Tw.tobytes() == cp.camera_motion.tobytes()
    carried = cp.frame_poses[0][0]
    assert carried.pose.tobytes() == _mat44_mul(Tw, T_obj).tobytes() and np.allclose(carried.t, carried.pose[:3, 3])
    assert abs(np.linalg.norm(carried.q) - 1) < 1e-12 and "track_camera" in cp.timings and cp.motion_stats["n_host_syncs"] == 1
    truth = T_cam @ T_obj
    d_start, d_carried = R.mean_row_error(model, T_obj, truth), R.mean_row_error(model, carried.pose, truth)
    cp.RefineFrame(depth=d2)
    row = cp.refine_info[0, 0]
    d_refined = R.mean_row_error(model, cp.frame_poses[0][0].pose, truth)
    print(f"ellipsoid: {d_start * 1e3:.2f} mm before, {d_carried * 1e3:.2f} mm carried by T, {d_refined * 1e3:.2f} mm refined; status {int(row['status'])}")
    assert row["status"] in (R.CONVERGED, R.MAX_ITERS) and d_refined <= 0.003
    assert d_carried < d_start
    # the refinement is the oracle's from the carried pose
    Tr, want = R.refine(model, _mat44_mul(Tw, T_obj), d2, intr)
    assert cp.frame_poses[0][0].pose.tobytes() == Tr.tobytes() and int(row["status"]) == want["status"]


def test_cpp_demo_matches_the_python_route(tmp_path):
    frames, _ = Cs.stream(3, seed=5, mm=15, deg=1.5, rows=66, cols=130)
    intr = Cs.intrinsics(66, 130)
    exe = str(tmp_path / "depth_motion_demo")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "depth_motion_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    np.concatenate([f.reshape(-1) for f in frames]).astype("<f4").tofile(str(tmp_path / "frames.f32"))
    p = dict(levels=3, iters=(6, 4, 3, 0))
    r = subprocess.run([exe, str(tmp_path / "frames.f32"), "3", "66", "130"] + [repr(float(v)) for v in intr] + ["3", "6", "4", "3", "0"],
                       check=True, capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    odo = DepthOdometry(66, 130, intr, params=p)
    odo.push(frames[0])
    fmt = lambda T: " ".join("%.17g" % v for v in np.asarray(T).reshape(-1))
    for k in (1, 2):
        T, info, st = device(frames[k - 1], frames[k], intr, p)
        assert f"pair {k} status {st['status']} evaluations {st['n_evaluations']} of {st['n_enqueued']} launches {st['n_launches']} syncs 1" in lines
        assert "  T " + fmt(T) in lines, (fmt(T), r.stdout)
        for l in range(3):
            row = info[l]
            assert (f"  level {l} status {row['status']} iterations {row['iterations']} size {row['rows']} x {row['cols']} source {row['n_source']} "
                    f"pairs {row['n_pairs_first']} -> {row['n_pairs_last']} rmse %.9g -> %.9g" % (float(row["rmse_first"]), float(row["rmse_last"]))) in lines
        odo.push(frames[k])
    assert lines[-1] == "pose " + fmt(odo.pose)
