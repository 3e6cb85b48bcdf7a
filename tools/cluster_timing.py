"""Time ppf_prep_clusters, the step that turns a plane-free scene into detections, against the plane removal in front of it
and against the scipy restatement it is held to.

Inputs:
  rendered  the two-bottle frame of tests/test_gpu_frame.py::_render_frame (360 x 640) after one plane: 18,010 rows, tolerance
            0.02 (the default), min_size 100
  c1        the reference's frame (tests/golden/c1_depth_window.npz) after two planes: 98,135 rows, tolerance 0.01, min_size 200
Routes, alternating in one process after a warm-up (median and spread of `--reps`), per input:
  remove_planes   scene.remove_planes(...)                        ppf_prep_planes, the call that precedes
  clusters        kept.clusters(params, intr, image size)         ppf_prep_clusters
and, timed once over `--oracle-reps` runs, cluster_oracle.clusters on the same rows (k-d tree pairs + connected components).
The device is checked against the oracle (info rows, counts, labels) on both inputs before anything is timed.  Writes
profiles/r17_cluster_timing.json (or --out).  The kernel trace is a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o clusters -- python tools/cluster_timing.py --reps 5 --no-write
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

import cluster_oracle as CL  # noqa: E402
import prep_data as D  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud  # noqa: E402


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
            t0 = time.perf_counter()
            out = fn()   # every entry waits for its kernels before it returns
            ms[key].append((time.perf_counter() - t0) * 1e3)
            del out
    return {k: summary(v) for k, v in ms.items()}


def stage(scene_rows, plane_params, params, intr, image_size, reps, oracle_reps):
    scene = DeviceCloud.upload(scene_rows)
    kept = scene.remove_planes(plane_params)
    rows = kept.rows()
    found, info, counts, labels, stats = kept.clusters(params, intr, image_size, return_info=True, return_labels=True)
    t = []
    for _ in range(oracle_reps):
        t0 = time.perf_counter()
        want = CL.clusters(rows, params, intr=intr, image_size=image_size)
        t.append((time.perf_counter() - t0) * 1e3)
    assert info.tobytes() == want[1].tobytes() and (counts == want[2]).all() and (labels == want[3]).all(), "the device differs from the oracle"
    doc = {"rows": len(scene), "rows_after_planes": len(kept), "params": params, "counts": [int(v) for v in counts],
           "cluster_rows": [int(v) for v in info["n_rows"][:int(counts[0])]],
           "boxes": [[int(v) for v in b] for b in info["box_xywh"][:int(counts[0])]],
           "counters": {k: v for k, v in stats.items() if k.startswith("n_")}, "oracle": summary(t)}
    doc.update(alternate({"remove_planes": lambda: scene.remove_planes(plane_params),
                          "clusters": lambda: kept.clusters(params, intr, image_size)}, reps))
    doc["clusters_over_remove_planes"] = round(doc["clusters"]["median_ms"] / doc["remove_planes"]["median_ms"], 3)
    doc["oracle_over_clusters"] = round(doc["oracle"]["median_ms"] / doc["clusters"]["median_ms"], 1)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--oracle-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_cluster_timing.json"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cluster_timing.py needs a GPU")
    doc = {"tool": "tools/cluster_timing.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps}
    from test_gpu_frame import _render_frame
    scene, depth, boxes, K, objs, solid = _render_frame(np.load(os.path.join(D.GOLDEN, "bottle_model_xyzn.npy")))
    doc["rendered"] = stage(scene, dict(n_hypotheses=256, max_planes=1), dict(tolerance=0.02, min_size=100),
                            (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])), depth.shape, a.reps, a.oracle_reps)
    xyz, depth, _, intr = D.c1_frame()
    doc["c1"] = stage(xyz, dict(n_hypotheses=256, max_planes=2), dict(tolerance=0.01, min_size=200), tuple(float(v) for v in intr),
                      depth.shape, a.reps, a.oracle_reps)
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
