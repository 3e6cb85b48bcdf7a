"""ppf_verify_frame on the device against a numpy restatement of DESIGN.md §14: every count and the fitness / support bits
equal the oracle's (inlier_rmse within one fp32 ulp) on the rendered frame and on the C1 chain; the scores order true
poses above perturbed ones; a pose's score row does not depend on the rest of the call; edge cases; two concurrent
callers; the Python and C++ wrappers."""
import ctypes as C
import math
import os
import subprocess
import threading

import numpy as np
import pytest
from scipy.spatial import cKDTree

import prep_data as D
from test_gpu_frame import _render_frame
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import FrameDetection, IcpParams, MatchFrameStats, Pose, check, lib
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, verify_frame
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEFAULTS = dict(leaf=0.003, mean_k=50, stddev_mul=1.0, normal_k=30, curvature_threshold=0.03)
F32 = np.float32
INT_FIELDS = ["n_rows", "n_considered", "n_inliers", "n_visible", "n_supported", "n_occluded", "n_violations"]


# ---- the oracle ------------------------------------------------------------------------------------------------------
def moved_rows(model, T, step):
    rows = np.ascontiguousarray(model[::step], dtype=F32)
    out = np.zeros_like(rows)
    Tm = (C.c_double * 16)(*np.asarray(T, dtype=np.float64).reshape(16).tolist())
    check(lib().ppf_transform_pc_pose(rows.ctypes.data, rows.shape[0], 6, 3, Tm, out.ctypes.data))
    return out


class Neighbours:
    """the candidate pairs (model row, scene row) of one moved cloud within a radius slightly above inlier_dist"""

    def __init__(self, o, scene, r):
        self.fin = np.isfinite(o).all(axis=1)
        sfin = np.isfinite(scene).all(axis=1)
        self.S = np.ascontiguousarray(scene[sfin], dtype=F32)
        qi = np.nonzero(self.fin)[0]
        if len(self.S) == 0 or len(qi) == 0:
            self.i = self.j = np.zeros(0, dtype=np.int64)
            return
        tree = cKDTree(self.S[:, :3].astype(np.float64))
        lists = tree.query_ball_point(o[qi, :3].astype(np.float64), r * 1.01 + 1e-6)
        lens = np.fromiter((len(v) for v in lists), dtype=np.int64, count=len(lists))
        self.i = np.repeat(qi, lens)
        self.j = np.fromiter((k for v in lists for k in v), dtype=np.int64, count=int(lens.sum()))


def oracle(o, nb, p, depth=None, intr=None):
    """the score row of one pose (a dict) from its moved rows o and their candidate pairs nb"""
    r2 = F32(p["inlier_dist"]) * F32(p["inlier_dist"])
    with np.errstate(all="ignore"):
        x, y, z, nx, ny, nz = (o[:, k] for k in range(6))
        facing = (nx.astype(np.float64) * x.astype(np.float64) + ny.astype(np.float64) * y.astype(np.float64)) + \
            nz.astype(np.float64) * z.astype(np.float64) < 0
        cons = nb.fin & (facing | bool(p["flags"] & _capi.PPF_VERIFY_ALL_ROWS))
        i, S = nb.i, nb.S
        sj = S[nb.j]
        dx, dy, dz = sj[:, 0] - x[i], sj[:, 1] - y[i], sj[:, 2] - z[i]
        d2 = (dx * dx + dy * dy) + dz * dz
        ok = (d2 <= r2) & cons[i]
        if p["flags"] & _capi.PPF_VERIFY_NORMALS:
            ok &= (nx[i] * sj[:, 3] + ny[i] * sj[:, 4]) + nz[i] * sj[:, 5] >= F32(p["normal_cos"])
        best = np.full(len(o), np.inf, dtype=F32)
        np.minimum.at(best, i[ok], d2[ok])
        inl = np.isfinite(best)
        n_vis = n_sup = n_occ = n_vio = 0
        if depth is not None:
            fx, fy, ppx, ppy = intr
            zz = cons & (z > 0)
            uf = x.astype(np.float64) * fx / z.astype(np.float64) + ppx
            vf = y.astype(np.float64) * fy / z.astype(np.float64) + ppy
            ui, vi = np.floor(uf + 0.5), np.floor(vf + 0.5)
            inr = zz & (ui >= 0) & (ui < depth.shape[1]) & (vi >= 0) & (vi < depth.shape[0])
            d = np.zeros(len(o), dtype=F32)
            d[inr] = depth[vi[inr].astype(np.int64), ui[inr].astype(np.int64)]
            vis = inr & np.isfinite(d) & (d > 0)
            e = (d - z).astype(F32)
            tol = F32(p["depth_tol"])
            n_vis = int(vis.sum())
            n_sup = int((vis & (np.abs(e) <= tol)).sum())
            n_occ = int((vis & (e < -tol)).sum())
            n_vio = int((vis & (e > tol)).sum())
    n_cons, n_inl = int(cons.sum()), int(inl.sum())
    out = dict(n_rows=len(o), n_considered=n_cons, n_inliers=n_inl, n_visible=n_vis, n_supported=n_sup, n_occluded=n_occ,
               n_violations=n_vio)
    out["inlier_rmse"] = F32(math.sqrt(float(best[inl].astype(np.float64).sum()) / n_inl)) if n_inl else F32(0)
    out["fitness"] = F32(n_inl / n_cons) if n_cons else F32(0)
    den = n_vis - n_occ
    out["support"] = F32(n_sup / den) if den else F32(0)
    out["score"] = out["support"] if depth is not None else out["fitness"]
    return out


def assert_row(got, want, what=""):
    for f in INT_FIELDS:
        assert int(got[f]) == want[f], (what, f, int(got[f]), want[f])
    for f in ("fitness", "support", "score"):
        assert F32(got[f]).tobytes() == F32(want[f]).tobytes(), (what, f, got[f], want[f])
    a, b = F32(got["inlier_rmse"]).view(np.int32), F32(want["inlier_rmse"]).view(np.int32)
    assert abs(int(a) - int(b)) <= 1, (what, "inlier_rmse", got["inlier_rmse"], want["inlier_rmse"])


def params(inlier_dist=0.005, depth_tol=0.01, model_step=1, flags=0, normal_cos=0.5):
    return dict(inlier_dist=inlier_dist, depth_tol=depth_tol, model_step=model_step, flags=flags, normal_cos=normal_cos)


def oracle_argmax(rows):
    s = [F32(r["score"]) for r in rows]
    return int(np.argmax(s)) if s else -1   # np.argmax: the first of equal maxima


# ---- fixtures -----------------------------------------------------------------------------------------------------------
def rot_about(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K


def shifted(T, v):
    S = T.copy()
    S[:3, 3] += v
    return S


def rotated(T, centre, R):
    """T followed by a rotation R about the scene point `centre`"""
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = centre - R @ centre
    return M @ T


@pytest.fixture(scope="module")
def rendered(bottle):
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    pairs = DeviceCloud.upload(scene).prep_frame(boxes, depth, intr, dict(DEFAULTS, leaf=0.004))
    models = [bottle, bottle, solid]
    clouds = {id(bottle): DeviceCloud.upload(bottle), id(solid): DeviceCloud.upload(solid)}
    return dict(depth=depth, intr=intr, K=K, objs=objs, solid=solid, models=models, objects=[o for o, _ in pairs],
                edges=[e for _, e in pairs], obj_rows=[o.rows() for o, _ in pairs], mclouds=[clouds[id(m)] for m in models])


def perturbations(T, model):
    """(label, pose): the true pose, +-5 / 10 / 30 mm along x and along the view ray, 10 and 90 degrees about the model centre"""
    c = T[:3, :3] @ model[:, :3].astype(np.float64).mean(axis=0) + T[:3, 3]
    ray = c / np.linalg.norm(c)
    out = [("true", T)]
    for mm in (5, 10, 30):
        for sgn in (1, -1):
            out.append((f"x{sgn * mm}", shifted(T, sgn * mm * 1e-3 * np.array([1.0, 0, 0]))))
            out.append((f"ray{sgn * mm}", shifted(T, sgn * mm * 1e-3 * ray)))
    for deg in (10, 90):
        out.append((f"rot{deg}", rotated(T, c, rot_about([0.3, 1.0, 0.2], deg))))
    return out


@pytest.fixture(scope="module")
def refined(rendered):
    """the rendered frame's detections through ppf_match_frame: their refined poses"""
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


def rendered_poses(rendered, refined):
    """per detection the scored poses: the perturbations of the true pose, then the refined ones"""
    return [[T for _, T in perturbations(rendered["objs"][i][1], rendered["models"][i])] + refined[i] for i in range(3)]


@pytest.fixture(scope="module")
def c1(bottle):
    xyz, depth, box, intr = D.c1_frame()
    pairs = DeviceCloud.upload(xyz).prep_frame([box, (5, 5, 10, 10)], depth, intr, DEFAULTS)
    golden = np.load(os.path.join(GOLDEN, "c1_pipeline_golden.npz"))
    assert len(pairs[1][0]) == 0   # the second box lies where the depth image is empty
    return dict(depth=depth, intr=intr, obj=pairs[0][0], obj_rows=pairs[0][0].rows(), empty=pairs[1][0], mcloud=DeviceCloud.upload(bottle),
                poses=[golden["icp_poses"][k] for k in range(5)])


def check_parity(models, scenes, poses_per_det, prm, depth=None, intr=None, dets=None, nbs=None):
    scores, best, st = verify_frame(dets, poses_per_det, None, depth, intr, prm)
    for i, plist in enumerate(poses_per_det):
        want = []
        for k, T in enumerate(plist):
            o = moved_rows(models[i], T, prm["model_step"])
            key = (i, k, prm["model_step"], prm["inlier_dist"])
            if nbs is None or key not in nbs:
                nb = Neighbours(o, scenes[i], prm["inlier_dist"])
                if nbs is not None:
                    nbs[key] = (o, nb)
            else:
                o, nb = nbs[key]
            want.append(oracle(o, nb, prm, depth, intr))
            assert_row(scores[i, k], want[-1], (i, k, prm))
        for k in range(len(plist), scores.shape[1]):
            assert scores[i, k].tobytes() == bytes(scores.dtype.itemsize)
        assert best[i] == oracle_argmax(want), (i, prm)
    return scores, best, st


# ---- 1. parity on the rendered frame -----------------------------------------------------------------------------------
SWEEP = [(r, s) for r in (0.002, 0.005, 0.02) for s in (1, 3)]


@pytest.mark.parametrize("inlier_dist,step", SWEEP)
def test_rendered_frame_parity(rendered, refined, inlier_dist, step):
    # 15 perturbations and up to 5 refined poses per object: each object appears twice, as two detections of one call
    poses = [[T for _, T in perturbations(rendered["objs"][i][1], rendered["models"][i])] for i in range(3)] + refined
    dets = [(rendered["mclouds"][i % 3], rendered["objects"][i % 3]) for i in range(6)]
    models, scenes = rendered["models"] * 2, rendered["obj_rows"] * 2
    nbs = {}
    n = 0
    for ncos in (None, 0.0, 0.9):
        for all_rows in (0, _capi.PPF_VERIFY_ALL_ROWS):
            for tol in (None, 0.005, 0.02):
                flags = all_rows | (_capi.PPF_VERIFY_NORMALS if ncos is not None else 0)
                prm = params(inlier_dist, tol or 0.01, step, flags, 0.5 if ncos is None else ncos)
                depth = rendered["depth"] if tol else None
                check_parity(models, scenes, poses, prm, depth, rendered["intr"] if tol else None, dets, nbs)
                n += 1
    assert n == 18


# ---- 2. the C1 chain -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_depth", [False, True])
def test_c1_golden_icp_poses(c1, bottle, use_depth):
    prm = params()
    depth = c1["depth"] if use_depth else None
    scores, best, st = check_parity([bottle], [c1["obj_rows"]], [c1["poses"]], prm, depth, c1["intr"] if use_depth else None,
                                    [(c1["mcloud"], c1["obj"])])
    assert st["n_jobs"] == 5 and st["n_dets"] == 1 and st["n_host_syncs"] == 1
    assert scores[0, 0]["n_inliers"] > 0


# ---- 3. geometry ---------------------------------------------------------------------------------------------------------
def axis_of(model, T):
    w, v = np.linalg.eigh(np.cov(model[:, :3].astype(np.float64).T))
    return T[:3, :3] @ v[:, -1]


@pytest.mark.parametrize("use_depth", [False, True])
def test_true_poses_score_above_perturbations(rendered, use_depth):
    prm = params(0.005, 0.005)
    depth = rendered["depth"] if use_depth else None
    intr = rendered["intr"] if use_depth else None
    for i in range(3):
        model, T = rendered["objs"][i]
        c = T[:3, :3] @ model[:, :3].astype(np.float64).mean(axis=0) + T[:3, 3]
        ray = c / np.linalg.norm(c)
        cands = []
        if i == 2:   # the box: every perturbation of >= 10 mm or >= 10 degrees
            cands = [(lab, P) for lab, P in perturbations(T, model) if lab != "true" and abs(int(lab.lstrip("xrayot"))) >= 10]
        else:        # a bottle: translations perpendicular to its axis, rotations about axes perpendicular to it
            ax = axis_of(model, T)
            u = np.cross(ax, ray)
            u /= np.linalg.norm(u)
            w = np.cross(ax, u)
            for mm in (10, 30):
                for sgn in (1, -1):
                    cands += [(f"u{sgn * mm}", shifted(T, sgn * mm * 1e-3 * u)), (f"w{sgn * mm}", shifted(T, sgn * mm * 1e-3 * w))]
            for deg in (10, 30, 90):
                cands += [(f"ru{deg}", rotated(T, c, rot_about(u, deg))), (f"rw{deg}", rotated(T, c, rot_about(w, deg)))]
        poses = [[T] + [P for _, P in cands]]
        scores, best, _ = verify_frame([(rendered["mclouds"][i], rendered["objects"][i])], poses, None, depth, intr, prm)
        s = scores[0]["score"]
        for k, (lab, _) in enumerate(cands):
            assert s[0] > s[k + 1], (i, use_depth, lab, s[0], s[k + 1])
        assert best[0] == 0


def test_depth_classes_in_front_and_behind(rendered):
    prm = params(0.005, 0.005)
    for i in range(3):
        model, T = rendered["objs"][i]
        c = T[:3, :3] @ model[:, :3].astype(np.float64).mean(axis=0) + T[:3, 3]
        ray = c / np.linalg.norm(c)
        poses = [[T, shifted(T, -0.03 * ray), shifted(T, 0.03 * ray)]]
        scores, _, _ = verify_frame([(rendered["mclouds"][i], rendered["objects"][i])], poses, None, rendered["depth"], rendered["intr"], prm)
        assert scores[0, 1]["n_violations"] > 0, i       # towards the camera: in front of the observed surface
        assert scores[0, 2]["n_occluded"] > 0, i         # away from it: behind the observed surface
        assert scores[0, 1]["n_violations"] > scores[0, 0]["n_violations"]
        assert scores[0, 2]["n_occluded"] > scores[0, 0]["n_occluded"]


# ---- 4. segmentation invariance and determinism --------------------------------------------------------------------------
def _alone_rows(entries, depth, intr, prm):
    return [verify_frame([d], [p], 5, depth, intr, prm)[0][0].tobytes() for d, p in entries]


def test_rows_do_not_depend_on_the_rest_of_the_call(c1, rendered, refined):
    prm = params()
    c1_entry = ((c1["mcloud"], c1["obj"]), c1["poses"])
    r_entries = [((rendered["mclouds"][i], rendered["objects"][i]), rendered_poses(rendered, refined)[i][:5]) for i in range(3)]
    # without depth: C1 x 1, 3, 8 mixed with the rendered detections
    alone_c1 = _alone_rows([c1_entry], None, None, prm)[0]
    alone_r = _alone_rows(r_entries, None, None, prm)
    launches = {}
    for K in (1, 3, 8):
        entries = [c1_entry] * K + r_entries if K > 1 else [c1_entry]
        scores, best, st = verify_frame([e[0] for e in entries], [e[1] for e in entries], 5, None, None, prm)
        for k in range(K):
            assert scores[k].tobytes() == alone_c1, K
        for j in range(3 if K > 1 else 0):
            assert scores[K + j].tobytes() == alone_r[j], (K, j)
        again = verify_frame([e[0] for e in entries], [e[1] for e in entries], 5, None, None, prm)
        assert again[0].tobytes() == scores.tobytes() and np.array_equal(again[1], best)
    for K in (1, 8):
        _, _, st = verify_frame([c1_entry[0]] * K, [c1_entry[1]] * K, 5, None, None, prm)
        launches[K] = (st["n_launches"], st["n_host_syncs"])
    assert launches[1] == launches[8] == (9, 1), launches   # grid count, five-launch scan, grid scatter, score, finish; the score rows
    # with depth: detections share one frame's image
    alone = _alone_rows([c1_entry], c1["depth"], c1["intr"], prm)[0]
    for K in (1, 3, 8):
        scores, _, st = verify_frame([c1_entry[0]] * K, [c1_entry[1]] * K, 5, c1["depth"], c1["intr"], prm)
        assert all(scores[k].tobytes() == alone for k in range(K)), K
        launches[K] = (st["n_launches"], st["n_host_syncs"])
    assert launches[1] == launches[8] == (9, 1), launches   # the depth image is an upload, not a launch
    alone_r = _alone_rows(r_entries, rendered["depth"], rendered["intr"], prm)
    scores, _, _ = verify_frame([e[0] for e in r_entries], [e[1] for e in r_entries], 5, rendered["depth"], rendered["intr"], prm)
    assert [scores[j].tobytes() for j in range(3)] == alone_r


# ---- 5. edge cases -------------------------------------------------------------------------------------------------------
def test_edge_cases(c1, bottle):
    prm = params()
    d = (c1["mcloud"], c1["obj"])
    T = c1["poses"][0]
    # all n_poses zero: nothing is launched
    scores, best, st = verify_frame([d, d, None], [[], [], []], 4, c1["depth"], c1["intr"], prm)
    assert list(best) == [-1, -1, -1] and not scores.tobytes().strip(b"\0") and st["n_launches"] == 0 and st["n_jobs"] == 0
    # an empty scene cloud: no inliers, the depth part still counted
    scores, best, _ = verify_frame([(c1["mcloud"], c1["empty"]), d], [[T], [T]], None, c1["depth"], c1["intr"], prm)
    assert scores[0, 0]["n_inliers"] == 0 and scores[0, 0]["inlier_rmse"] == 0 and scores[0, 0]["n_visible"] > 0
    for f in ("n_considered", "n_visible", "n_supported", "n_occluded", "n_violations", "support", "score"):
        assert scores[0, 0][f] == scores[1, 0][f], f
    assert scores[1, 0]["n_inliers"] > 0
    # a NaN pose and a pose that puts the model behind the camera
    nan = T.copy()
    nan[0, 1] = np.nan
    behind = shifted(T, np.array([0, 0, -3.0]))
    scores, best, _ = verify_frame([d], [[nan, behind, T]], None, c1["depth"], c1["intr"], prm)
    n = bottle.shape[0]
    assert scores[0, 0]["n_rows"] == n and all(scores[0, 0][f] == 0 for f in INT_FIELDS[1:])
    assert scores[0, 0]["score"] == 0 and scores[0, 0]["fitness"] == 0
    assert scores[0, 1]["n_visible"] == 0 and scores[0, 1]["score"] == 0
    assert best[0] == 2
    # model_step beyond the model: one row
    scores, _, _ = verify_frame([d], [[T]], None, None, None, params(model_step=n + 5))
    assert scores[0, 0]["n_rows"] == 1
    o = moved_rows(bottle, T, n + 5)
    assert_row(scores[0, 0], oracle(o, Neighbours(o, c1["obj_rows"], 0.005), params(model_step=n + 5)))


def test_two_concurrent_callers(c1, rendered, refined):
    prm = params()
    a = ([(c1["mcloud"], c1["obj"])] * 4, [c1["poses"]] * 4, c1["depth"], c1["intr"])
    polys = rendered_poses(rendered, refined)
    b = ([(rendered["mclouds"][i], rendered["objects"][i]) for i in range(3)] * 2, [p[:8] for p in polys] * 2, None, None)
    want = [verify_frame(x[0], x[1], 8, x[2], x[3], prm)[0].tobytes() for x in (a, b)]
    got, errs = [None, None], []
    start = threading.Barrier(2)

    def run(k, x):
        try:
            start.wait()
            for _ in range(4):
                r = verify_frame(x[0], x[1], 8, x[2], x[3], prm)[0].tobytes()
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


# ---- 6. the CloudProcessor wrapper ---------------------------------------------------------------------------------------
def test_pose_validation_wrapper(bottle):
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    labels = ["bottle", "bottle", "box"]
    cp = CloudProcessor(scene, depth, boxes, [39, 39, 73], [0, 1, 2], 0.05, 0.05)
    cp.LoadSingleModel(bottle, "bottle")
    cp.LoadSingleModel(solid, "box")
    cp.TrainDetector(0.05, 0.05)
    cp.PrepareFrame(K, 0.004, 50, 1.0, 30, 0.03)
    first = cp.MatchFrame(labels)
    poses_before = [[p.pose.copy() for p in lst] for lst in cp.frame_poses]
    chosen = cp.PoseValidation()
    assert "pose_validation" in cp.timings and cp.verify_stats["n_dets"] == 3
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    prm = params()
    models = [bottle, bottle, solid]
    for i in range(3):
        assert len(cp.frame_poses[i]) > 0 and first[i] is not None
        np.testing.assert_array_equal(cp.frame_poses[i][0].pose, first[i].pose)
        want = []
        for P in cp.frame_poses[i]:
            o = moved_rows(models[i], P.pose, 1)
            want.append(oracle(o, Neighbours(o, cp.object_mats[i].rows(), 0.005), prm, depth, intr))
            assert_row(cp.pose_scores[i, len(want) - 1], want[-1], i)
        assert cp.best_index[i] == oracle_argmax(want)
        assert chosen[i] is cp.frame_poses[i][cp.best_index[i]]
    # min_score between the lowest best score and the next higher one: exactly the lowest become None
    bests = sorted({float(cp.pose_scores[i, cp.best_index[i]]["score"]) for i in range(3)})
    assert len(bests) >= 2, bests
    cut = (bests[0] + bests[1]) / 2
    cut_out = cp.PoseValidation(min_score=cut)
    for i in range(3):
        low = float(cp.pose_scores[i, cp.best_index[i]]["score"]) == bests[0]
        assert (cut_out[i] is None) == low and (low or cut_out[i] is chosen[i]), i
    # MatchFrame's own result is the same with or without the validation after it; the loop route keeps the same poses
    again = cp.MatchFrame(labels)
    for p, q in zip(first, again):
        assert pose_bytes(p) == pose_bytes(q)
    loop = cp.MatchFrame(labels, one_pass=False)
    assert [[p.pose.tobytes() for p in lst] for lst in cp.frame_poses] == [[a.tobytes() for a in lst] for lst in poses_before]
    assert [pose_bytes(p) for p in loop] == [pose_bytes(p) for p in first]
    assert [pose_bytes(p) for p in cp.PoseValidation()] == [pose_bytes(p) for p in chosen]
    # no depth: fitness ranks
    cp.PoseValidation(use_depth=False)
    assert all(cp.pose_scores[i, k]["n_visible"] == 0 and cp.pose_scores[i, k]["score"] == cp.pose_scores[i, k]["fitness"]
               for i in range(3) for k in range(len(cp.frame_poses[i])))


def pose_bytes(p):
    return None if p is None else bytes(p.to_record())


# ---- 7. the C++ facade ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compiler", ["g++", "clang++"])
def test_cpp_facade_verify_frame(tmp_path, bottle, compiler):
    xyz, depth, box, intr = D.c1_frame()
    x, y, w, h = box
    boxes = np.asarray([box, (x - 10, y - 15, w + 30, h + 25), box], np.int32)
    exe = str(tmp_path / "frame_verify_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "frame_verify_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}",
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
    cp.MatchFrame(["bottle"] * 3)
    dets = [(cp._model_clouds[0], cp.object_mats[i]) for i in range(3)]
    scores, best, _ = verify_frame(dets, cp.frame_poses, 5, depth, intr, params())
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3, r.stdout
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
