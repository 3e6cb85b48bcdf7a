"""Time ppf_prep_planes, the step in front of the crop, against the calls around it.

Inputs:
  c1        the reference's frame (tests/golden/c1_depth_window.npz): 166,718 rows, one box
  dense     a seeded 720 x 1280 frame without an invalid pixel: a tilted plane with a dozen boxes standing on it, four boxes
  rendered  the two-bottle frame of tests/test_gpu_frame.py::_render_frame (360 x 640), for the chain
Routes, alternating in one process after a warm-up (median and spread of `--reps`), per input:
  cloud_from_depth   DeviceCloud.from_depth(host image)                     a yardstick: one pass over the image
  remove_planes      scene.remove_planes(256 hypotheses, one plane)         ppf_prep_planes
  prep_frame         scene.prep_frame(boxes)                                the yardstick: the call the stage precedes
  prep_frame_after   kept.prep_frame(boxes)                                 the same call on what the stage leaves
and on `rendered` PrepareFrame + MatchFrame with and without RemovePlanes in front (the removal's time included).
remove_planes is checked against tests/plane_oracle.py on `rendered` before anything is timed.  Writes
profiles/r16_plane_timing.json (or --out).  The kernel trace is a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o planes -- python tools/plane_timing.py --reps 5 --no-write
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plane_oracle as P  # noqa: E402
import prep_data as D  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud  # noqa: E402

PARAMS = dict(n_hypotheses=256, max_planes=1)
FRAME = dict(leaf=0.003, mean_k=50, stddev_mul=1.0, normal_k=30, curvature_threshold=0.03)


def dense_frame(rng, rows=720, cols=1280):
    fx = fy = 900.0
    ppx, ppy = cols / 2 - 0.5, rows / 2 - 0.5
    vv, uu = np.mgrid[0:rows, 0:cols]
    ray = np.stack([(uu - ppx) / fx, (vv - ppy) / fy, np.ones_like(uu, dtype=np.float64)], axis=-1)
    nrm = np.array([0.05, -0.5, -0.86]) / np.linalg.norm([0.05, -0.5, -0.86])
    depth = -0.9 / (ray @ nrm)
    depth += rng.normal(scale=0.0007, size=depth.shape)   # sensor noise, well inside the 5 mm threshold
    boxes = []
    for k in range(12):
        r0, c0 = int(rng.integers(60, rows - 200)), int(rng.integers(60, cols - 200))
        h, w = int(rng.integers(60, 140)), int(rng.integers(60, 140))
        depth[r0:r0 + h, c0:c0 + w] -= rng.uniform(0.05, 0.15)
        if k < 4:
            boxes.append((c0, r0, w, h))
    return depth.astype(np.float32), boxes, (fx, fy, ppx, ppy)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()   # every entry waits for its kernels before it returns
    return out, (time.perf_counter() - t0) * 1e3


def summary(v):
    v = np.asarray(v)
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
            "p90_ms": round(float(np.percentile(v, 90)), 4)}


def alternate(routes, reps):
    for _ in range(3):
        for fn in routes.values():
            fn()
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for key, fn in routes.items():
            out, dt = timed(fn)
            ms[key].append(dt)
            del out
    return {k: summary(v) for k, v in ms.items()}


def stage_routes(depth, boxes, intr, reps):
    scene = DeviceCloud.from_depth(depth, intr)
    kept, info, stats = scene.remove_planes(PARAMS, return_info=True)
    routes = {"cloud_from_depth": lambda: DeviceCloud.from_depth(depth, intr),
              "remove_planes": lambda: scene.remove_planes(PARAMS),
              "prep_frame": lambda: scene.prep_frame(boxes, depth, intr, FRAME),
              "prep_frame_after": lambda: kept.prep_frame(boxes, depth, intr, FRAME)}
    doc = {"shape": list(depth.shape), "rows": len(scene), "rows_kept": len(kept), "boxes": len(boxes),
           "plane": {"n": [round(float(v), 6) for v in info[0]["n"]], "d": round(float(info[0]["d"]), 6), "status": int(info[0]["status"]),
                     "n_inliers": int(info[0]["n_inliers"]), "refit": int(info[0]["refit"])},
           "counters": {k: v for k, v in stats.items() if k.startswith("n_")}}
    doc.update(alternate(routes, reps))
    doc["remove_planes_over_prep_frame"] = round(doc["remove_planes"]["median_ms"] / doc["prep_frame"]["median_ms"], 3)
    doc["saved_in_prep_frame_ms"] = round(doc["prep_frame"]["median_ms"] - doc["prep_frame_after"]["median_ms"], 4)
    return doc


def chain(reps):
    from test_gpu_frame import _render_frame
    bottle = np.load(os.path.join(D.GOLDEN, "bottle_model_xyzn.npy"))
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    got = DeviceCloud.upload(scene).remove_planes(PARAMS, return_info=True, return_labels=True)
    want = P.remove_planes(scene, PARAMS)
    assert got[1].tobytes() == want[2].tobytes() and (got[2] == want[3]).all(), "the device differs from the oracle"
    labels = ["bottle", "bottle", "box"]
    cps = {}
    for remove in (False, True):
        cp = CloudProcessor(scene, depth, boxes, [39, 39, 73], [0, 1, 2], 0.05, 0.05)
        cp.LoadSingleModel(bottle, "bottle")
        cp.LoadSingleModel(solid, "box")
        cp.TrainDetector(0.05, 0.05)
        cps[remove] = (cp, cp.scene)

    def run(remove):
        cp, full = cps[remove]
        cp.scene = full
        if remove:
            cp.RemovePlanes(**PARAMS)
        cp.PrepareFrame(K, 0.004, 50, 1.0, 30, 0.03)
        return cp.MatchFrame(labels)
    doc = alternate({"prep_match": lambda: run(False), "remove_prep_match": lambda: run(True)}, reps)
    for remove, key in ((False, "prep_match"), (True, "remove_prep_match")):
        cp = cps[remove][0]
        doc[key]["crop_rows"] = [int(v) for v in cp.stage_rows[:, 0]]
        doc[key]["best_votes"] = [int(f[0].numVotes) if f else 0 for f in cp.frame_poses]
    doc["remove_planes_alone"] = alternate({"remove_planes": lambda: cps[True][1].remove_planes(PARAMS)}, reps)["remove_planes"]
    doc["saved_ms"] = round(doc["prep_match"]["median_ms"] - doc["remove_prep_match"]["median_ms"], 4)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_plane_timing.json"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("plane_timing.py needs a GPU")
    doc = {"tool": "tools/plane_timing.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps,
           "params": PARAMS}
    _, depth, box, intr = D.c1_frame()
    doc["c1"] = stage_routes(depth, [box], intr, a.reps)
    depth, boxes, intr = dense_frame(np.random.default_rng(16))
    doc["dense"] = stage_routes(depth, boxes, intr, a.reps)
    doc["rendered_chain"] = chain(a.reps)
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
