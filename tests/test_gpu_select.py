"""ppf_select_frame on the device against the numpy restatement of DESIGN.md §16 (tests/select_oracle.py): every info field,
the selection and both images byte for byte, on the oracle poses of the two-bottle frame (tests/golden/select_two_bottles.npz)
and on the C1 frame's five golden poses as five detections, over the overlap limits, splat radii, depth tolerances, pixel
gates, with and without verify scores (one of them NaN); skipped detections, NaN, clipped and behind-the-camera poses; two
instances inside one detection; isolation, constant launch and sync counts, two concurrent callers, the Python and C++
wrappers, and the whole chain on the device ending in exactly one pose per bottle."""
import ctypes as C
import itertools
import os
import subprocess
import threading

import numpy as np
import pytest

import prep_data as D
import select_oracle as S
from test_gpu_frame import _render_frame
from test_gpu_verify import DEFAULTS, F32, moved_rows, params, shifted
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import FrameDetection, IcpParams, MatchFrameStats, Pose, check, lib
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, select_frame, verify_frame_rendered
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
RP = dict(splat_radius=0.003, visible_tol=0.005)
TOP = 8
UNION = (72, 142, 309, 83)


# ---- fixtures ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame(bottle):
    """the two-bottle frame, its three boxes prepared on the device, and the oracle poses of the fixture"""
    scene, depth, boxes, K, objs, _ = _render_frame(bottle)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    boxes = [boxes[0], boxes[1], UNION]
    fx = np.load(os.path.join(GOLDEN, "select_two_bottles.npz"))
    assert fx["boxes"].tolist() == [list(b) for b in boxes]
    pairs = DeviceCloud.upload(scene).prep_frame(boxes, depth, intr, dict(DEFAULTS, leaf=0.004))
    poses = [[fx["poses"][i, k] for k in range(int(fx["n_poses"][i]))] for i in range(3)]
    return dict(scene=scene, depth=depth, intr=intr, K=K, boxes=boxes, pairs=pairs, objects=[o for o, _ in pairs], poses=poses,
                true=[objs[0][1], objs[1][1]], mcloud=DeviceCloud.upload(bottle), cache={})


@pytest.fixture(scope="module")
def c1(bottle):
    xyz, depth, box, intr = D.c1_frame()
    pairs = DeviceCloud.upload(xyz).prep_frame([box], depth, intr, DEFAULTS)
    golden = np.load(os.path.join(GOLDEN, "c1_pipeline_golden.npz"))
    return dict(depth=depth, intr=tuple(float(v) for v in intr), obj=pairs[0][0], mcloud=DeviceCloud.upload(bottle),
                poses=[golden["icp_poses"][k] for k in range(5)], cache={})


# ---- the comparison -----------------------------------------------------------------------------------------------------
def oracle(models, poses, top, depth, intr, rp, sp, scores=None, cache=None):
    hyps = [(i * top + k, moved_rows(models[i], T, 1)) for i, plist in enumerate(poses) if models[i] is not None
            for k, T in enumerate(plist)]
    keys = None if scores is None else scores["score"].reshape(-1)
    return S.select(hyps, len(poses) * top, depth, intr, rp["splat_radius"], keys=keys, cache=cache, **dict(S.DEFAULTS, **sp))


def check_select(models, mclouds, poses, depth, intr, rp, sp, scores=None, top=None, cache=None):
    """one device call against the oracle: info, selected, n_selected and both images, byte for byte"""
    info, sel, img, lab, st = select_frame(mclouds, poses, depth, intr, sp, rp, scores, top, return_images=True, return_stats=True)
    want = oracle(models, poses, info.shape[1], depth, intr, rp, sp, scores, cache)
    what = (rp, sp, scores is not None)
    wi = want["info"].reshape(info.shape)
    for f in S.INFO.names:
        assert info[f].tobytes() == wi[f].tobytes(), (f, what, info[f], wi[f])
    assert info.tobytes() == wi.tobytes(), what
    assert sel.tolist() == want["selected"][:want["n_selected"]].tolist(), what
    assert st["n_selected"] == want["n_selected"] == len(sel) and st["n_eligible"] == want["n_eligible"], what
    assert img.tobytes() == want["depth"].tobytes(), (what, int((img != want["depth"]).sum()))
    assert np.array_equal(lab, want["label"]), (what, int((lab != want["label"]).sum()))
    assert st["n_host_syncs"] <= 2 and st["n_jobs"] == sum(len(p) for m, p in zip(models, poses) if m is not None)
    return info, sel, img, lab, st, want


def sweep(models, mclouds, poses, depth, intr, radius, scores, cache):
    """the parity parameters: max_overlap x depth_tol x min_pixels x {explained, scores}, at one splat radius"""
    rp = dict(RP, splat_radius=radius)
    seen = set()
    for mo, tol, mp, sc in itertools.product((0.0, 0.25, 1.0), (0.003, 0.01), (1, 2000), (None, scores)):
        sp = dict(max_overlap=mo, depth_tol=tol, min_pixels=mp)
        info, sel, _, _, st, want = check_select(models, mclouds, poses, depth, intr, rp, sp, sc, scores.shape[1], cache)
        seen.add(tuple(sel.tolist()))
        if mo == 1.0:    # nothing conflicts: every eligible hypothesis is selected
            assert st["n_selected"] == st["n_eligible"] and not (info["status"] == S.SUPPRESSED).any()
        if mo == 0.0:    # any shared supported pixel conflicts
            for a, b in itertools.combinations(sel.tolist(), 2):
                assert np.intersect1d(want["supported"][a], want["supported"][b]).size == 0, (a, b)
            assert (info["n_overlap"][info["status"] == S.SUPPRESSED] > 0).all()
        assert (info["n_supported"][info["status"] != S.GATED].reshape(-1) >= mp).all()
        if sc is not None:   # the planted NaN score is gated, whatever its pixels say
            nan = np.isnan(sc["score"])
            assert nan.sum() == 1 and (info["status"][nan] == S.GATED).all() and np.isnan(info["key"][nan]).all()
    return seen


def frame_scores(frame):
    dets = [(frame["mcloud"], frame["objects"][i]) for i in range(3)]
    scores, _, _ = verify_frame_rendered(dets, frame["poses"], TOP, frame["depth"], frame["intr"], params(), RP)
    return scores


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0.003, 0.0015])
def test_select_parity_two_bottles(frame, bottle, radius):
    scores = frame_scores(frame)
    scores[0, 0]["score"] = np.nan   # the best hypothesis of bottle 0: its duplicate (0, 3) has to take its place
    seen = sweep([bottle] * 3, [frame["mcloud"]] * 3, frame["poses"], frame["depth"], frame["intr"], radius, scores, frame["cache"])
    assert len(seen) >= 3, seen   # the sweep is not degenerate: the limits 0, 0.25 and 1 select different sets


@pytest.mark.parametrize("radius", [0.003, 0.0015])
def test_select_parity_c1_five_detections(c1, bottle, radius):
    dets = [(c1["mcloud"], c1["obj"])] * 5
    poses = [[P] for P in c1["poses"]]
    scores, _, _ = verify_frame_rendered(dets, poses, 1, c1["depth"], c1["intr"], params(), RP)
    scores[3, 0]["score"] = np.nan
    seen = sweep([bottle] * 5, [c1["mcloud"]] * 5, poses, c1["depth"], c1["intr"], radius, scores, c1["cache"])
    assert len(seen) >= 2, seen
    # the same five poses as one detection with top 5: the same counts under other flat indices
    a = select_frame([c1["mcloud"]], [c1["poses"]], c1["depth"], c1["intr"], None, RP)[0]
    b = select_frame([c1["mcloud"]] * 5, poses, c1["depth"], c1["intr"], None, RP)[0]
    for f in ("n_drawn", "n_supported", "explained", "status", "rank"):
        assert a[0][f].tobytes() == b[:, 0][f].tobytes(), f


def test_the_gate_leaves_one_pose_per_bottle(frame, bottle):
    """the figures of the issue on the device: with min_score 0.3 exactly (0, 0) and (1, 0), whatever the overlap limit"""
    for mo in (0.1, 0.25, 0.5):
        info, sel, _, lab, _, _ = check_select([bottle] * 3, [frame["mcloud"]] * 3, frame["poses"], frame["depth"], frame["intr"], RP,
                                               dict(min_score=0.3, max_overlap=mo), cache=frame["cache"])
        assert sel.tolist() == [0, TOP], (mo, sel)
        assert info[0, 0]["explained"] >= 0.79 and info[1, 0]["explained"] >= 0.79
        assert info[2, 0]["explained"] <= 0.18 and info[2, 4]["explained"] <= 0.18
        assert set(np.unique(lab)) == {-1, 0, TOP}
    info, sel, *_ = check_select([bottle] * 3, [frame["mcloud"]] * 3, frame["poses"], frame["depth"], frame["intr"], RP, {},
                                 cache=frame["cache"])
    assert sel.tolist() == [0, TOP, 2 * TOP + 4, 1]
    assert info[0, 3]["status"] == S.SUPPRESSED and info[0, 3]["suppressed_by"] == 0   # equal keys: the lower j wins


# ---- 2. skipped detections, NaN, clipped and behind-the-camera poses ------------------------------------------------------------
def test_skipped_nan_clipped_and_behind(c1, bottle):
    depth, intr, T = c1["depth"], c1["intr"], c1["poses"][0]
    c = T[:3, :3] @ bottle[:, :3].astype(np.float64).mean(axis=0) + T[:3, 3]
    nan = T.copy()
    nan[1, 2] = np.nan
    edge = shifted(T, np.array([-c[0] - intr[2] * c[2] / intr[0], 0.0, 0.0]))   # the centre on the image's left edge (u = 0)
    straddle = shifted(T, np.array([0.0, 0.0, -c[2]]))                          # the centre at z = 0: half behind the camera
    behind = shifted(T, np.array([0.0, 0.0, -2.0 * c[2]]))                      # all of it behind the camera
    poses = [[T, nan, edge, straddle], [T, T], [], [behind, c1["poses"][1]]]
    mclouds = [c1["mcloud"], None, c1["mcloud"], c1["mcloud"]]
    models = [bottle, None, bottle, bottle]
    for sp in ({}, dict(max_overlap=0.0), dict(max_overlap=1.0, min_pixels=50)):
        info, sel, img, lab, st, _ = check_select(models, mclouds, poses, depth, intr, RP, sp, cache=c1["cache"])
        assert st["n_jobs"] == 6 and st["n_dets"] == 4
        assert not info[1].tobytes().strip(b"\0") and not info[2].tobytes().strip(b"\0")   # no model cloud; no poses
        assert not info[3, 2:].tobytes().strip(b"\0")
        for i, k in ((0, 1), (3, 0)):   # the NaN pose and the pose behind the camera draw nothing
            r = info[i, k]
            assert (r["status"], r["rank"], r["suppressed_by"], r["n_drawn"], r["n_supported"], r["n_overlap"]) == (S.GATED, -1, -1, 0, 0, 0)
            assert r["explained"] == 0 and r["key"] == 0
        assert info[0, 2]["n_drawn"] > 0 and info[0, 3]["n_drawn"] > 0   # clipped by the border; half behind the camera
        assert 0 < info[0, 2]["n_drawn"] < info[0, 0]["n_drawn"]
        assert len(sel) >= 1 and info.reshape(-1)[sel[0]]["rank"] == 0
    # nothing at all: no device work, empty outputs
    info, sel, img, lab, st = select_frame([None, c1["mcloud"]], [[T], []], depth, intr, None, RP, return_images=True, return_stats=True)
    assert sel.size == 0 and not info.tobytes().strip(b"\0") and (img == 0).all() and (lab == -1).all()
    assert st["n_launches"] == 0 and st["n_host_syncs"] == 0 and st["n_jobs"] == 0
    info, sel = select_frame([], [], depth, intr, None, RP)
    assert info.shape[0] == 0 and sel.size == 0


# ---- 3. two instances inside one detection --------------------------------------------------------------------------------------
def test_two_instances_in_one_detection(frame, bottle):
    """the union box alone: its poses hold both bottles, and label_out shows both -- one pose per detection cannot"""
    info, sel, img, lab, st, _ = check_select([bottle], [frame["mcloud"]], [frame["poses"][2]], frame["depth"], frame["intr"], RP,
                                              dict(min_score=0.3), cache=frame["cache"])
    assert sel.tolist() == [1, 2] and st["n_dets"] == 1
    assert (lab == 1).sum() > 500 and (lab == 2).sum() > 500 and set(np.unique(lab)) == {-1, 1, 2}
    for j, (x, y, w, h) in zip(sel.tolist(), frame["boxes"][:2]):   # each instance over its own bottle
        vv, uu = np.nonzero(lab == j)
        assert x <= uu.mean() <= x + w and y <= vv.mean() <= y + h, (j, uu.mean(), vv.mean())
    assert (img[lab >= 0] > 0).all() and (img[lab < 0] == 0).all()


# ---- 4. isolation, launch and sync counts, concurrency ---------------------------------------------------------------------------
def test_counts_do_not_depend_on_the_rest_of_the_call(frame):
    mc, depth, intr = frame["mcloud"], frame["depth"], frame["intr"]
    full, _, st24 = select_frame([mc] * 3, frame["poses"], depth, intr, None, RP, return_stats=True)
    assert st24["n_jobs"] == 24
    counts = set()
    for i, k in ((0, 0), (0, 3), (1, 0), (1, 3), (2, 0), (2, 4), (0, 1), (2, 7)):
        one, sel, st1 = select_frame([mc], [[frame["poses"][i][k]]], depth, intr, None, RP, return_stats=True)
        for f in ("n_drawn", "n_supported", "explained"):
            assert one[0, 0][f].tobytes() == full[i, k][f].tobytes(), (i, k, f)
        counts.add((st1["n_launches"], st1["n_host_syncs"]))
    counts.add((st24["n_launches"], st24["n_host_syncs"]))
    assert counts == {(7, 2)}, counts   # window, splat, mask, key, overlap, greedy, report; the windows and the results
    # with the images: two more launches, the same for 1 and 24 hypotheses
    a = select_frame([mc], [frame["poses"][0][:1]], depth, intr, None, RP, return_images=True, return_stats=True)[-1]
    b = select_frame([mc] * 3, frame["poses"], depth, intr, None, RP, return_images=True, return_stats=True)[-1]
    assert (a["n_launches"], a["n_host_syncs"]) == (b["n_launches"], b["n_host_syncs"]) == (9, 2)   # + paint and resolve


def test_two_concurrent_callers(frame, c1):
    def call(x):
        out = select_frame(x[0], x[1], x[2], x[3], x[4], RP, return_images=True)
        return b"".join(np.ascontiguousarray(o).tobytes() for o in out)

    jobs = [([frame["mcloud"]] * 3, frame["poses"], frame["depth"], frame["intr"], dict(min_score=0.3)),
            ([c1["mcloud"]] * 5, [[P] for P in c1["poses"]], c1["depth"], c1["intr"], dict(max_overlap=0.0))]
    want = [call(x) for x in jobs]
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


# ---- 5. the chain on the device ------------------------------------------------------------------------------------------------
def device_poses(frame, bottle, top=TOP):
    det = PPF3DDetector(0.05, 0.05).trainModel(bottle)
    dets = (FrameDetection * 3)()
    for i, (obj, edge) in enumerate(frame["pairs"]):
        dets[i].model, dets[i].model_cloud = det._model.ptr, frame["mcloud"]._ptr
        dets[i].scene, dets[i].edge = obj._ptr, edge._ptr
    ip = IcpParams()
    lib().ppf_default_icp_params(C.byref(ip))
    out, n_out = (Pose * (3 * top))(), (C.c_int * 3)()
    check(lib().ppf_match_frame(dets, 3, C.byref(det._params(0.05, 0.05, False)), C.byref(ip), top, out, n_out, None,
                                C.byref(MatchFrameStats())))
    return [[np.array(out[i * top + k].pose).reshape(4, 4) for k in range(n_out[i])] for i in range(3)]


def test_end_to_end_on_the_device(frame, bottle):
    """_render_frame -> prep_frame on the three boxes -> ppf_match_frame, top 8 -> ppf_select_frame, min_score 0.3: the
    oracle's result on the device's own poses, exactly two hypotheses, one within 3 mm of each bottle's true pose (the CPU
    oracles' poses lie 1.5 mm from them: the bound is twice that)."""
    poses = device_poses(frame, bottle)
    assert all(len(p) > 0 for p in poses)
    info, sel, img, lab, st, _ = check_select([bottle] * 3, [frame["mcloud"]] * 3, poses, frame["depth"], frame["intr"], RP,
                                              dict(min_score=0.3), top=TOP)
    model = bottle[:, :3].astype(np.float64)
    dist = np.array([[np.linalg.norm((model @ poses[j // TOP][j % TOP][:3, :3].T + poses[j // TOP][j % TOP][:3, 3]) -
                                     (model @ T[:3, :3].T + T[:3, 3]), axis=1).mean() for T in frame["true"]] for j in sel.tolist()])
    print("selected", sel.tolist(), "explained", [float(info.reshape(-1)[j]["explained"]) for j in sel.tolist()], "distances (m)", dist.tolist())
    assert len(sel) == 2, (sel, dist)
    assert sorted(dist.argmin(axis=1).tolist()) == [0, 1], dist
    assert (dist.min(axis=1) <= 0.003).all(), dist


# ---- 6. the wrappers ------------------------------------------------------------------------------------------------------------
def test_cloud_processor_select_frame(frame, bottle):
    depth, intr = frame["depth"], frame["intr"]
    cp = CloudProcessor(frame["scene"], depth, frame["boxes"], [39] * 3, [0, 1, 2], 0.05, 0.05)
    cp.LoadSingleModel(bottle, "bottle")
    cp.TrainDetector(0.05, 0.05)
    cp.PrepareFrame(frame["K"], 0.004, 50, 1.0, 30, 0.03)
    cp.MatchFrame(["bottle", "bottle", None])
    chosen, img, lab = cp.SelectFrame(min_score=0.3, return_images=True)
    mats = [[P.pose for P in plist] for plist in cp.frame_poses]
    assert mats[2] == [] and len(mats[0]) > 0 and len(mats[1]) > 0
    info, sel, wimg, wlab, _, _ = check_select([bottle, bottle, None], [frame["mcloud"], frame["mcloud"], None], mats, depth, intr, RP,
                                               dict(min_score=0.3))
    top = info.shape[1]
    assert cp.select_info.tobytes() == info.tobytes() and [(i * top + k) for i, k in cp.selected] == sel.tolist()
    assert [(i, k) for i, k, _ in chosen] == cp.selected and all(P is cp.frame_poses[i][k] for i, k, P in chosen)
    assert img.tobytes() == wimg.tobytes() and np.array_equal(lab, wlab)
    assert len(chosen) == 2 and {i for i, _, _ in chosen} == {0, 1}
    assert cp.select_stats["n_host_syncs"] <= 2 and "select_frame" in cp.timings
    # ranked by the rendered verification's score
    with pytest.raises(_capi.PPFError):
        cp.SelectFrame(use_scores=True)
    cp.PoseValidation(visibility="rendered")
    cp.SelectFrame(min_score=0.3, use_scores=True)
    want = select_frame([frame["mcloud"], frame["mcloud"], None], mats, depth, intr, dict(min_score=0.3), RP, cp.pose_scores)
    assert cp.select_info.tobytes() == want[0].tobytes() and cp.select_info[0, 0]["key"] == cp.pose_scores[0, 0]["score"]
    with pytest.raises(_capi.PPFError):
        select_frame([frame["mcloud"]], [mats[0]], None, intr)
    with pytest.raises(_capi.PPFError):
        select_frame([frame["mcloud"]], [mats[0]], depth, intr, dict(max_overlap=1.5))


@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_cpp_facade_select_frame(tmp_path, frame, bottle, compiler):
    scene, depth, intr = frame["scene"], frame["depth"], frame["intr"]
    boxes = np.asarray(frame["boxes"], np.int32)
    exe = str(tmp_path / "frame_select_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frame_select_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}",
                    "-o", exe], check=True)
    (tmp_path / "scene.f32").write_bytes(np.ascontiguousarray(scene, np.float32).tobytes())
    (tmp_path / "depth.f32").write_bytes(np.ascontiguousarray(depth, np.float32).tobytes())
    (tmp_path / "boxes.i32").write_bytes(boxes.tobytes())
    (tmp_path / "model.f32").write_bytes(np.ascontiguousarray(bottle, np.float32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "scene.f32"), str(scene.shape[0]), str(tmp_path / "depth.f32"), str(depth.shape[0]),
                        str(depth.shape[1])] + [repr(float(v)) for v in intr] +
                       [str(tmp_path / "boxes.i32"), str(len(boxes)), str(tmp_path / "model.f32"), str(bottle.shape[0]),
                        str(tmp_path / "out_depth.f32"), str(tmp_path / "out_label.i32"), "0.3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the demo's chain from Python: prepareFrame's default stages (leaf 3 mm), matchFrame with top 8
    pairs = DeviceCloud.upload(scene).prep_frame(frame["boxes"], depth, intr, DEFAULTS)
    poses = device_poses(dict(frame, pairs=pairs), bottle)
    top = max(len(p) for p in poses)
    info, sel, img, lab = select_frame([frame["mcloud"]] * 3, poses, depth, intr, dict(min_score=0.3), RP, return_images=True)
    lines = r.stdout.strip().splitlines()
    n = sum(len(p) for p in poses)
    assert len(lines) == n + len(sel) + 1, r.stdout
    names = ["status", "rank", "suppressed_by", "n_drawn", "n_supported", "n_overlap", "explained", "key"]
    at = 0
    for i, plist in enumerate(poses):
        for k in range(len(plist)):
            f = lines[at].split()
            at += 1
            assert f[:3] == ["pose", str(i), f"{k}:"] and f[3::2] == names, lines[at - 1]
            for name, v in zip(names, f[4::2]):
                if name in ("explained", "key"):
                    assert F32(float(v)).tobytes() == F32(info[i, k][name]).tobytes(), (i, k, name)
                else:
                    assert int(v) == int(info[i, k][name]), (i, k, name)
    for rnk, j in enumerate(sel.tolist()):
        assert lines[at + rnk] == f"selected {rnk}: det {j // top} k {j % top}", lines[at + rnk]
    assert lines[-1] == f"eligible {int((info['status'] % 2 == 1).sum())} selected {len(sel)}"
    assert (tmp_path / "out_depth.f32").read_bytes() == img.tobytes()
    assert (tmp_path / "out_label.i32").read_bytes() == lab.tobytes()
