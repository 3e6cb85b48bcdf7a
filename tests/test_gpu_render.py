"""ppf_render_frame and ppf_verify_frame_rendered on the device against the numpy restatement of DESIGN.md §15
(tests/render_oracle.py): the depth and label images bit for bit, every count and the fitness / support bits of the
rendered verification (inlier_rmse within one fp32 ulp), the considered rows a subset of ppf_verify_frame's, the old entry
again with an unbounded tolerance, self-occlusion found on a tilted torus and not on convex solids, isolation, two
concurrent callers, and the Python and C++ wrappers."""
import ctypes as C
import math
import os
import subprocess
import threading

import numpy as np
import pytest

import prep_data as D
import render_oracle as R
from test_gpu_frame import _render_frame
from test_gpu_verify import (DEFAULTS, F32, INT_FIELDS, Neighbours, assert_row, moved_rows, oracle, oracle_argmax, params, perturbations,
                             rendered_poses, shifted)
from yolo_ppf_pose_estimation_amd import _capi, synth
from yolo_ppf_pose_estimation_amd._capi import FrameDetection, IcpParams, MatchFrameStats, Pose, check, lib
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, render_frame, verify_frame, verify_frame_rendered
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
RP = dict(splat_radius=0.003, visible_tol=0.005)


# ---- fixtures ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rendered(bottle):
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    pairs = DeviceCloud.upload(scene).prep_frame(boxes, depth, intr, dict(DEFAULTS, leaf=0.004))
    models = [bottle, bottle, solid]
    clouds = {id(bottle): DeviceCloud.upload(bottle), id(solid): DeviceCloud.upload(solid)}
    return dict(depth=depth, intr=intr, K=K, objs=objs, solid=solid, models=models, objects=[o for o, _ in pairs],
                edges=[e for _, e in pairs], obj_rows=[o.rows() for o, _ in pairs], mclouds=[clouds[id(m)] for m in models])


@pytest.fixture(scope="module")
def refined(rendered):
    det_b = PPF3DDetector(0.05, 0.05).trainModel(rendered["models"][0])
    det_s = PPF3DDetector(0.05, 0.05).trainModel(rendered["solid"])
    dets = (FrameDetection * 3)()
    for i, d in enumerate((det_b, det_b, det_s)):
        dets[i].model, dets[i].model_cloud = d._model.ptr, rendered["mclouds"][i]._ptr
        dets[i].scene, dets[i].edge = rendered["objects"][i]._ptr, rendered["edges"][i]._ptr
    ip = IcpParams()
    lib().ppf_default_icp_params(C.byref(ip))
    out, n_out = (Pose * 15)(), (C.c_int * 3)()
    check(lib().ppf_match_frame(dets, 3, C.byref(det_b._params(0.05, 0.05, False)), C.byref(ip), 5, out, n_out, None,
                                C.byref(MatchFrameStats())))
    return [[np.array(out[i * 5 + k].pose).reshape(4, 4) for k in range(n_out[i])] for i in range(3)]


@pytest.fixture(scope="module")
def c1(bottle):
    xyz, depth, box, intr = D.c1_frame()
    pairs = DeviceCloud.upload(xyz).prep_frame([box], depth, intr, DEFAULTS)
    golden = np.load(os.path.join(GOLDEN, "c1_pipeline_golden.npz"))
    return dict(depth=depth, intr=tuple(float(v) for v in intr), obj=pairs[0][0], obj_rows=pairs[0][0].rows(),
                mcloud=DeviceCloud.upload(bottle), poses=[golden["icp_poses"][k] for k in range(5)])


# ---- the oracle of the rendered verification ------------------------------------------------------------------------------
def rendered_oracle(model, scene, T, prm, rp, shape, intr, depth=None, cache=None):
    """the score row of one pose: ppf_verify_frame's oracle with a row considered only where its own render sees it"""
    key = (id(model), np.asarray(T).tobytes(), prm["model_step"], prm["inlier_dist"], rp["splat_radius"], rp["visible_tol"])
    if cache is not None and key in cache:
        o, nb = cache[key]
    else:
        full = moved_rows(model, T, 1)
        vis = R.visible(full, R.zbuffer(full, shape[0], shape[1], intr, rp["splat_radius"]), intr, rp["visible_tol"])
        o = np.ascontiguousarray(full[::prm["model_step"]])
        nb = Neighbours(o, scene, prm["inlier_dist"])
        nb.fin = nb.fin & vis[::prm["model_step"]]
        if cache is not None:
            cache[key] = (o, nb)
    return oracle(o, nb, prm, depth, intr if depth is not None else None)


def check_rendered(models, scenes, dets, poses, prm, rp, shape, intr, depth=None, cache=None):
    scores, best, st = verify_frame_rendered(dets, poses, None, depth, intr, prm, rp, image_size=shape)
    for i, plist in enumerate(poses):
        want = []
        for k, T in enumerate(plist):
            want.append(rendered_oracle(models[i], scenes[i], T, prm, rp, shape, intr, depth, cache))
            assert_row(scores[i, k], want[-1], (i, k, prm, rp))
        for k in range(len(plist), scores.shape[1]):
            assert scores[i, k].tobytes() == bytes(scores.dtype.itemsize)
        assert best[i] == oracle_argmax(want), (i, prm)
    return scores, best, st


def frame_oracle(chosen, shape, intr, radius):
    """chosen: per detection (model, pose) or None -> the oracle's (depth, label)"""
    return R.render_frame([(i, moved_rows(m, T, 1)) for i, c in enumerate(chosen) if c is not None for m, T in [c]], shape[0], shape[1],
                          intr, radius)


def assert_images(got, want, what=""):
    assert got[0].tobytes() == want[0].tobytes(), (what, int((got[0] != want[0]).sum()))
    assert np.array_equal(got[1], want[1]), (what, int((got[1] != want[1]).sum()))


# ---- 1. render parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0.003, 0.0015])
def test_render_frame_parity_rendered_frame(rendered, radius):
    shape, intr = rendered["depth"].shape, rendered["intr"]
    poses = [[T] for _, T in rendered["objs"]]
    got = render_frame(rendered["mclouds"], poses, [0, 0, 0], shape[0], shape[1], intr, dict(RP, splat_radius=radius), return_stats=True)
    want = frame_oracle([(m, T) for m, T in rendered["objs"]], shape, intr, radius)
    assert_images(got, want)
    for i in range(3):
        assert (got[1] == i).sum() > 500, i
    st = got[2]
    assert st["n_jobs"] == 3 and st["n_dets"] == 3 and st["n_host_syncs"] == 1 and st["n_launches"] == 2
    # skipped detections and None entries draw nothing
    got = render_frame([rendered["mclouds"][0], None, rendered["mclouds"][2]], poses, [-1, 0, 0], shape[0], shape[1], intr,
                       dict(RP, splat_radius=radius))
    assert_images(got, frame_oracle([None, None, rendered["objs"][2]], shape, intr, radius))


@pytest.mark.parametrize("radius", [0.003, 0.0015])
def test_render_frame_parity_c1(c1, bottle, radius):
    shape, intr = c1["depth"].shape, c1["intr"]
    # five detections, one golden ICP pose each: they overlap, so the label tie-break and the least depth both matter
    got = render_frame([c1["mcloud"]] * 5, [c1["poses"]] * 5, [0, 1, 2, 3, 4], shape[0], shape[1], intr, dict(RP, splat_radius=radius))
    assert_images(got, frame_oracle([(bottle, c1["poses"][k]) for k in range(5)], shape, intr, radius))
    # one detection drawn twice at the same pose: every pixel goes to the lower index
    got = render_frame([c1["mcloud"]] * 2, [c1["poses"][:1]] * 2, [0, 0], shape[0], shape[1], intr, dict(RP, splat_radius=radius))
    assert set(np.unique(got[1])) == {-1, 0}


def test_render_frame_parity_clipped_and_behind(c1, bottle):
    shape, intr = c1["depth"].shape, c1["intr"]
    T = c1["poses"][0]
    c = T[:3, :3] @ bottle[:, :3].astype(np.float64).mean(axis=0) + T[:3, 3]
    edge = shifted(T, np.array([-c[0] - intr[2] * c[2] / intr[0], 0.0, 0.0]))   # the centre on the image's left edge (u = 0)
    straddle = shifted(T, np.array([0.0, 0.0, -c[2]]))                          # the centre at z = 0: half behind the camera
    near = shifted(T, np.array([0.0, 0.0, 0.2 - c[2]]))                           # close: the splats reach PPF_RENDER_MAX_SPLAT
    for P in (edge, straddle, near):
        got = render_frame([c1["mcloud"]], [[P]], [0], shape[0], shape[1], intr, RP)
        assert_images(got, frame_oracle([(bottle, P)], shape, intr, RP["splat_radius"]))
        assert (got[1] == 0).any()
    full = moved_rows(bottle, straddle, 1)
    assert (full[:, 2] < 0).any() and (full[:, 2] > 0).any()
    scores, _, _ = verify_frame_rendered([(c1["mcloud"], c1["obj"])], [[edge, straddle, near]], None, c1["depth"], intr, params(), RP)
    for k, P in enumerate((edge, straddle, near)):
        assert_row(scores[0, k], rendered_oracle(bottle, c1["obj_rows"], P, params(), RP, shape, intr, c1["depth"]), k)


# ---- 2. + 3. verify parity and the subset --------------------------------------------------------------------------------
def split_rendered(rendered, refined):
    """the rendered frame's 15 perturbations and up to 5 refined poses per object: each object as two detections of one call"""
    poses = [[T for _, T in perturbations(rendered["objs"][i][1], rendered["models"][i])] for i in range(3)] + refined
    dets = [(rendered["mclouds"][i % 3], rendered["objects"][i % 3]) for i in range(6)]
    return poses, dets, rendered["models"] * 2, rendered["obj_rows"] * 2


@pytest.mark.parametrize("step", [1, 3])
def test_verify_rendered_parity_rendered_frame(rendered, refined, step):
    shape, intr = rendered["depth"].shape, rendered["intr"]
    poses, dets, models, scenes = split_rendered(rendered, refined)
    cache = {}
    for flags, ncos in ((0, 0.5), (_capi.PPF_VERIFY_NORMALS, 0.5)):
        for use_depth in (False, True):
            prm = params(0.005, 0.01, step, flags, ncos)
            depth = rendered["depth"] if use_depth else None
            got, best, st = check_rendered(models, scenes, dets, poses, prm, RP, shape, intr, depth, cache)
            assert st["n_host_syncs"] == 2
            old, _, _ = verify_frame(dets, poses, None, depth, intr if use_depth else None, prm)
            for i in range(6):
                for k in range(len(poses[i])):
                    for f in INT_FIELDS[1:]:
                        assert int(got[i, k][f]) <= int(old[i, k][f]), (i, k, f)
                    assert got[i, k]["n_rows"] == old[i, k]["n_rows"]


@pytest.mark.parametrize("use_depth", [False, True])
def test_verify_rendered_parity_c1(c1, bottle, use_depth):
    shape, intr = c1["depth"].shape, c1["intr"]
    depth = c1["depth"] if use_depth else None
    for flags in (0, _capi.PPF_VERIFY_NORMALS):
        for rp in (RP, dict(splat_radius=0.0015, visible_tol=0.002)):
            prm = params(flags=flags)
            got, best, st = check_rendered([bottle], [c1["obj_rows"]], [(c1["mcloud"], c1["obj"])], [c1["poses"]], prm, rp, shape, intr,
                                           depth)
            old, _, _ = verify_frame([(c1["mcloud"], c1["obj"])], [c1["poses"]], None, depth, intr if use_depth else None, prm)
            for k in range(5):
                for f in INT_FIELDS[1:]:
                    assert int(got[0, k][f]) <= int(old[0, k][f]), (k, f)
                assert got[0, k]["n_considered"] < old[0, k]["n_considered"], k   # the bottle hides some of its facing rows
            assert st["n_jobs"] == 5 and st["n_host_syncs"] == 2


# ---- 4. an unbounded tolerance is the old entry -----------------------------------------------------------------------------
def test_unbounded_tolerance_reduces_to_verify_frame(c1, rendered, refined, bottle):
    cases = [([(c1["mcloud"], c1["obj"])], [c1["poses"]], [bottle], c1["depth"], c1["intr"])]
    poses, dets, models, _ = split_rendered(rendered, refined)
    cases.append((dets, poses, models, rendered["depth"], rendered["intr"]))
    rp = dict(splat_radius=0.003, visible_tol=1e30)
    n_all = n_kept = 0
    for dets, poses, models, depth, intr in cases:
        kept = []
        for i, plist in enumerate(poses):   # the poses of which every facing finite row is drawn and lands in the image
            kept.append([])
            for T in plist:
                o = moved_rows(models[i], T, 1)
                f = np.isfinite(o).all(axis=1) & R.facing(o)
                ren, ui, vi = R.centre(o, intr)
                if (ren & (ui >= 0) & (ui < depth.shape[1]) & (vi >= 0) & (vi < depth.shape[0]))[f].all():
                    kept[-1].append(T)
            n_all, n_kept = n_all + len(plist), n_kept + len(kept[-1])
        poses = kept
        for use_depth in (False, True):
            for flags in (0, _capi.PPF_VERIFY_NORMALS):
                prm = params(flags=flags)
                img = depth if use_depth else None
                a = verify_frame_rendered(dets, poses, None, img, intr, prm, rp, image_size=depth.shape)
                b = verify_frame(dets, poses, None, img, intr if use_depth else None, prm)
                assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    assert n_kept >= 0.8 * n_all, (n_kept, n_all)


# ---- 5. self-occlusion found --------------------------------------------------------------------------------------------
SYN = (360, 640, 460.0, 460.0, 319.5, 179.5)


def _tilt(deg, c=(0.0, 0.0, 0.6)):
    t = math.radians(deg)
    Rx = np.array([[1, 0, 0], [0, math.cos(t), -math.sin(t)], [0, math.sin(t), math.cos(t)]])
    T = np.eye(4)
    T[:3, :3] = Rx
    T[:3, 3] = np.asarray(c) - Rx @ np.asarray(c)
    return T


def _solid_frame(kind, deg):
    """one solid in front of a plane, drawn as _render_frame draws its objects; the solid's object cloud and its true pose"""
    rows, cols, fx, fy, ppx, ppy = SYN
    vv, uu = np.mgrid[0:rows, 0:cols]
    ray = np.stack([(uu - ppx) / fx, (vv - ppy) / fy, np.ones_like(uu, dtype=np.float64)], axis=-1)
    nrm, off = np.array([0.1, -0.15, -1.0]) / np.linalg.norm([0.1, -0.15, -1.0]), -0.95
    depth = (off / (ray @ nrm)).astype(np.float32)
    model = synth.make_solid(kind, 20000, seed=7)
    T = _tilt(deg)
    obj = synth.apply_pose(model, T)[:, :3].astype(np.float64)
    pu = np.round(obj[:, 0] / obj[:, 2] * fx + ppx).astype(int)
    pv = np.round(obj[:, 1] / obj[:, 2] * fy + ppy).astype(int)
    order = np.argsort(-obj[:, 2])
    for du in (0, 1):
        for dv in (0, 1):
            depth[np.clip(pv[order] + dv, 0, rows - 1), np.clip(pu[order] + du, 0, cols - 1)] = obj[order, 2]
    box = (int(pu.min()), int(pv.min()), int(pu.max() - pu.min()), int(pv.max() - pv.min()))
    zz = depth.astype(np.float64)
    scene = np.stack([(uu - ppx) * zz / fx, (vv - ppy) * zz / fy, zz], axis=-1).reshape(-1, 3).astype(np.float32)
    intr = (fx, fy, ppx, ppy)
    obj_cloud = DeviceCloud.upload(scene).prep_frame([box], depth, intr, dict(DEFAULTS, leaf=0.004))[0][0]
    return model, T, depth, intr, obj_cloud


@pytest.mark.parametrize("kind,deg,lo,hi", [("torus", 85, 0.30, 1.0), ("box", 30, 0.0, 0.01), ("cylinder", 50, 0.0, 0.05),
                                            ("cylinder", 70, 0.0, 0.05)])
def test_self_occlusion_found(kind, deg, lo, hi):
    model, T, depth, intr, obj = _solid_frame(kind, deg)
    mc = DeviceCloud.upload(model)
    prm = params()
    new, _, _ = verify_frame_rendered([(mc, obj)], [[T]], None, depth, intr, prm, RP)
    old, _, _ = verify_frame([(mc, obj)], [[T]], None, depth, intr, prm)
    a, b = int(new[0, 0]["n_considered"]), int(old[0, 0]["n_considered"])
    lost = 1.0 - a / b
    assert lo <= lost <= hi, (kind, deg, a, b, lost)
    assert_row(new[0, 0], rendered_oracle(model, obj.rows(), T, prm, RP, depth.shape, intr, depth), kind)
    if kind == "torus":
        assert new[0, 0]["fitness"] > old[0, 0]["fitness"], (new[0, 0]["fitness"], old[0, 0]["fitness"])


# ---- 6. isolation, NaN poses, concurrency ------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_rest_of_the_call(c1, rendered, refined):
    prm = params()
    shape, intr = c1["depth"].shape, c1["intr"]
    c1d = (c1["mcloud"], c1["obj"])
    alone = verify_frame_rendered([c1d], [c1["poses"]], 5, c1["depth"], intr, prm, RP)[0][0].tobytes()
    launches = set()
    for K in (1, 3, 8):
        scores, best, st = verify_frame_rendered([c1d] * K, [c1["poses"]] * K, 5, c1["depth"], intr, prm, RP)
        assert all(scores[k].tobytes() == alone for k in range(K)), K
        launches.add((st["n_launches"], st["n_host_syncs"]))
    assert launches == {(11, 2)}, launches   # the seven of the grids, window, splat, score, finish; the windows and the score rows
    # without depth, mixed with other poses (the render image is the same size)
    alone = verify_frame_rendered([c1d], [c1["poses"][2:3]], 5, None, intr, prm, RP, image_size=shape)[0][0, 0].tobytes()
    nan = c1["poses"][0].copy()
    nan[1, 2] = np.nan
    mixed = [c1["poses"][0], nan, c1["poses"][2], shifted(c1["poses"][1], np.array([0, 0, 0.3]))]
    scores, best, _ = verify_frame_rendered([c1d, None, c1d], [mixed, [], c1["poses"][2:3]], 5, None, intr, prm, RP, image_size=shape)
    assert scores[2, 0].tobytes() == alone
    assert all(scores[0, 1][f] == 0 for f in INT_FIELDS[1:]) and scores[0, 1]["n_rows"] > 0 and scores[0, 1]["score"] == 0
    assert best[1] == -1 and not scores[1].tobytes().strip(b"\0")
    # the render of one detection does not depend on the others' presence where they do not cover it
    shape_r, intr_r = rendered["depth"].shape, rendered["intr"]
    full = render_frame(rendered["mclouds"], [[T] for _, T in rendered["objs"]], [0, 0, 0], shape_r[0], shape_r[1], intr_r, RP)
    one = render_frame([None, rendered["mclouds"][1], None], [[], [rendered["objs"][1][1]], []], [-1, 0, -1], shape_r[0], shape_r[1],
                       intr_r, RP)
    m = one[1] == 1
    assert np.array_equal(full[1][m], one[1][m]) and full[0][m].tobytes() == one[0][m].tobytes()


def test_two_concurrent_callers(c1, rendered, refined):
    prm = params()
    a = ("v", [(c1["mcloud"], c1["obj"])] * 4, [c1["poses"]] * 4, c1["depth"], c1["intr"])
    polys = rendered_poses(rendered, refined)
    b = ("r", rendered["mclouds"], [[T] for _, T in rendered["objs"]], None, rendered["intr"], rendered["depth"].shape)

    def call(x):
        if x[0] == "v":
            return verify_frame_rendered(x[1], x[2], 8, x[3], x[4], prm, RP)[0].tobytes()
        d, l = render_frame(x[1], x[2], [0, 0, 0], x[5][0], x[5][1], x[4], RP)
        return d.tobytes() + l.tobytes()

    c = ("v", [(rendered["mclouds"][i], rendered["objects"][i]) for i in range(3)], [p[:8] for p in polys], None, rendered["intr"])
    jobs = [a, b]
    want = [call(x) for x in jobs]
    want_c = verify_frame_rendered(c[1], c[2], 8, None, c[4], prm, RP, image_size=rendered["depth"].shape)[0].tobytes()
    got, errs = [None, None], []
    start = threading.Barrier(2)

    def run(k, x):
        try:
            start.wait()
            for _ in range(4):
                if call(x) != want[k]:
                    got[k] = b"differs"
                    return
            got[k] = want[k]
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(k, x)) for k, x in enumerate(jobs)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert got == want
    assert verify_frame_rendered(c[1], c[2], 8, None, c[4], prm, RP, image_size=rendered["depth"].shape)[0].tobytes() == want_c


# ---- 7. the wrappers --------------------------------------------------------------------------------------------------------
def test_cloud_processor_rendered_validation_and_render(bottle):
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    labels = ["bottle", "bottle", "box"]
    cp = CloudProcessor(scene, depth, boxes, [39, 39, 73], [0, 1, 2], 0.05, 0.05)
    cp.LoadSingleModel(bottle, "bottle")
    cp.LoadSingleModel(solid, "box")
    cp.TrainDetector(0.05, 0.05)
    cp.PrepareFrame(K, 0.004, 50, 1.0, 30, 0.03)
    cp.MatchFrame(labels)
    facing = cp.PoseValidation()
    facing_scores = cp.pose_scores.copy()
    chosen = cp.PoseValidation(visibility="rendered")
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    dets = [(cp._model_clouds[cp.label_to_id[n]], cp.object_mats[i]) for i, n in enumerate(labels)]
    scores, best, st = verify_frame_rendered(dets, cp.frame_poses, None, depth, intr, params(), RP)
    assert cp.pose_scores.tobytes() == scores.tobytes() and cp.best_index == [int(b) for b in best]
    assert cp.verify_stats["n_host_syncs"] == 2
    models = [bottle, bottle, solid]
    for i in range(3):
        assert chosen[i] is cp.frame_poses[i][best[i]]
        for k, P in enumerate(cp.frame_poses[i]):
            assert_row(scores[i, k], rendered_oracle(models[i], cp.object_mats[i].rows(), P.pose, params(), RP, depth.shape, intr, depth))
            assert scores[i, k]["n_considered"] <= facing_scores[i, k]["n_considered"]
    assert len(facing) == 3
    img, lab = cp.RenderFrame()
    want = render_frame([d[0] for d in dets], cp.frame_poses, list(best), depth.shape[0], depth.shape[1], intr, RP)
    assert_images((img, lab), want)
    assert_images((img, lab), frame_oracle([(models[i], cp.frame_poses[i][best[i]].pose) for i in range(3)], depth.shape, intr, 0.003))
    assert cp.render_stats["n_jobs"] == 3 and "render_frame" in cp.timings
    # a min_score above every best keeps nothing: an empty render
    cp.PoseValidation(min_score=2.0, visibility="rendered")
    img, lab = cp.RenderFrame()
    assert (lab == -1).all() and (img == 0).all()
    with pytest.raises(_capi.PPFError):
        cp.PoseValidation(visibility="rendered", all_rows=True)
    with pytest.raises(_capi.PPFError):
        cp.PoseValidation(visibility="zbuffer")


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_cpp_facade_render_frame(tmp_path, bottle, compiler):
    xyz, depth, box, intr = D.c1_frame()
    x, y, w, h = box
    boxes = np.asarray([box, (x - 10, y - 15, w + 30, h + 25), box], np.int32)
    exe = str(tmp_path / "frame_render_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frame_render_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}",
                    "-o", exe], check=True)
    (tmp_path / "scene.f32").write_bytes(np.ascontiguousarray(xyz, np.float32).tobytes())
    (tmp_path / "depth.f32").write_bytes(np.ascontiguousarray(depth, np.float32).tobytes())
    (tmp_path / "boxes.i32").write_bytes(boxes.tobytes())
    (tmp_path / "model.f32").write_bytes(np.ascontiguousarray(bottle, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "scene.f32"), str(xyz.shape[0]), str(tmp_path / "depth.f32"), str(depth.shape[0]),
                        str(depth.shape[1])] + [repr(float(v)) for v in intr] +
                       [str(tmp_path / "boxes.i32"), str(len(boxes)), str(tmp_path / "model.f32"), str(bottle.shape[0]),
                        str(tmp_path / "out_depth.f32"), str(tmp_path / "out_label.i32")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    Kmat = np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1.0]])
    cp = CloudProcessor(xyz, depth, [tuple(int(v) for v in b) for b in boxes], [39] * 3, [0] * 3, 0.025, 0.05)
    cp.LoadSingleModel(bottle, "bottle")
    cp.TrainDetector(0.025, 0.05)
    cp.PrepareFrame(Kmat, 0.003, 50, 1.0, 30, 0.03)
    cp.MatchFrame(["bottle"] * 3)
    dets = [(cp._model_clouds[0], cp.object_mats[i]) for i in range(3)]
    scores, best, _ = verify_frame_rendered(dets, cp.frame_poses, 5, depth, intr, params(), RP)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 6, r.stdout
    for i in range(3):
        f = lines[i].split()
        assert f[0] == "det" and int(f[1].rstrip(":")) == i and f[2] == "best" and int(f[3]) == best[i], lines[i]
        vals = f[4:]
        row = scores[i, best[i]]
        names = vals[0::2]
        assert names == INT_FIELDS + ["inlier_rmse", "fitness", "support", "score"], names
        for name, v in zip(names, vals[1::2]):
            if name.startswith("n_"):
                assert int(v) == int(row[name]), name
            else:
                assert F32(float(v)).tobytes() == F32(row[name]).tobytes(), name
    img, lab = render_frame([d[0] for d in dets], cp.frame_poses, list(best), depth.shape[0], depth.shape[1], intr, RP)
    assert (tmp_path / "out_depth.f32").read_bytes() == img.tobytes()
    assert (tmp_path / "out_label.i32").read_bytes() == lab.tobytes()
    for i in range(3):
        assert lines[3 + i] == f"render {i}: pixels {int((lab == i).sum())}", lines[3 + i]
