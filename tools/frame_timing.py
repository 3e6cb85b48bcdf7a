"""Time the preparation of a frame with K detections, per-box chain against one ppf_prep_frame call.

The C1 frame (tests/golden/c1_depth_window.npz) with K = 1, 2, 4, 8, 16 boxes: the C1 box plus copies shifted by
multiples of 40 px.  Each K is warmed up, then the two routes alternate in the same process (median of `--reps`).
Writes profiles/r05_frame_timing.json.  The kernel trace is a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o frame -- python tools/frame_timing.py --reps 3 --no-write
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

import prep_data as D  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud  # noqa: E402

P = dict(leaf=0.003, mean_k=50, stddev_mul=1.0, normal_k=30, curvature_threshold=0.03)


def boxes_for(k, box, shape):
    x, y, w, h = box
    H, W = shape
    out = []
    for i in range(k):
        dx, dy = 40 * ((i + 1) // 2) * (1 if i % 2 else -1), 40 * (i // 4) * (1 if i % 8 < 4 else -1)
        bx, by = max(0, min(x + dx, W - 2)), max(0, min(y + dy, H - 2))
        out.append((bx, by, min(w, W - 1 - bx), min(h, H - 1 - by)))
    return out


def per_box(scene, boxes, depth, intr):
    out = []
    for b in boxes:
        n = scene.crop(b, depth, intr).voxel_grid(P["leaf"]).outlier_removal(P["mean_k"], P["stddev_mul"]).normals(P["normal_k"])
        out.append((n.to_mat(), n.edges(P["curvature_threshold"]).to_mat()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_frame_timing.json"))
    a = ap.parse_args()
    xyz, depth, box, intr = D.c1_frame()
    scene = DeviceCloud.upload(xyz)
    res = {"frame_points": int(xyz.shape[0]), "params": P, "reps": a.reps, "k": []}
    for k in (1, 2, 4, 8, 16):
        boxes = boxes_for(k, box, depth.shape)
        for _ in range(3):   # warm-up: block cache, code objects
            per_box(scene, boxes, depth, intr)
            scene.prep_frame(boxes, depth, intr, P)
        tb, tf = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            pb = per_box(scene, boxes, depth, intr)
            tb.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            fr, rows, st = scene.prep_frame(boxes, depth, intr, P, return_info=True)
            tf.append((time.perf_counter() - t0) * 1e3)
        same = all(np.array_equal(x[0].rows(), y[0].rows()) and np.array_equal(x[1].rows(), y[1].rows()) for x, y in zip(pb, fr))
        row = {"K": k, "per_box_ms": float(np.median(tb)), "frame_ms": float(np.median(tf)),
               "per_box_ms_min": float(np.min(tb)), "frame_ms_min": float(np.min(tf)),
               "speedup": float(np.median(tb) / np.median(tf)), "frame_n_launches": st["n_launches"],
               "frame_n_host_syncs": st["n_host_syncs"], "frame_ms_wall_lib": st["ms_wall"], "identical": bool(same),
               "rows_after_edges": [int(v) for v in rows[:, 3]]}
        res["k"].append(row)
        print(json.dumps(row), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
