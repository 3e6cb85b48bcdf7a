"""Time ppf_prep_regions against ppf_prep_clusters, the existing entry it stands beside, on the same cloud at the same tolerance.

Inputs, the two frames of tests/test_region_oracle.py, both with the normals and curvature of ppf_cloud_from_depth_normals:
  rendered  the two-bottle frame of tests/test_gpu_frame.py::_render_frame (360 x 640), background and all: 230,400 rows,
            tolerance 0.01, min_size 100
  c1        the reference's frame (tests/golden/c1_depth_window.npz) after two planes: 98,135 rows, tolerance 0.01, min_size 200
Routes, alternating in one process after a warm-up (median and spread of `--reps`), per input:
  clusters        cloud.clusters(tolerance, min_size, intr, image size)    ppf_prep_clusters
  regions         cloud.regions(the same, the other fields default)        ppf_prep_regions
The device is checked against the oracles (info rows, counts, labels) on both inputs and both routes before anything is timed.
Writes profiles/r19_region_timing.json (or --out).  The kernel trace is a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o regions -- python tools/region_timing.py --reps 5 --no-write
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
import region_oracle as R  # noqa: E402
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
    return ms


def stage(cloud, params, intr, image_size, reps):
    rows, curv = cloud.download()
    cp = dict(tolerance=params["tolerance"], min_size=params["min_size"])
    found, info, counts, labels, stats = cloud.regions(params, intr, image_size, return_info=True, return_labels=True)
    want = R.regions(rows, params, curv, intr, image_size)
    assert info.tobytes() == want[1].tobytes() and (counts == want[2]).all() and (labels == want[3]).all(), "regions: the device differs from the oracle"
    _, cinfo, ccounts, clabels, cstats = cloud.clusters(cp, intr, image_size, return_info=True, return_labels=True)
    want = CL.clusters(rows, cp, curv, intr, image_size)
    assert cinfo.tobytes() == want[1].tobytes() and (ccounts == want[2]).all() and (clabels == want[3]).all(), "clusters: the device differs from the oracle"
    smooth, border = R.kinds(rows, curv, R.params(params)["curvature_threshold"])
    doc = {"rows": len(cloud), "smooth_rows": int(smooth.sum()), "border_rows": int(border.sum()), "params": R.params(params),
           "counts": [int(v) for v in counts], "region_rows": [int(v) for v in info["n_rows"][:int(counts[0])]],
           "cluster_counts": [int(v) for v in ccounts], "cluster_rows": [int(v) for v in cinfo["n_rows"][:int(ccounts[0])]],
           # every union that succeeds takes one set away: smooth rows - components of them succeed, whatever the order
           "unions_succeeded": int(smooth.sum()) - int(counts[2]),
           "counters": {k: v for k, v in stats.items() if k.startswith("n_")},
           "cluster_counters": {k: v for k, v in cstats.items() if k.startswith("n_")}}
    ms = alternate({"clusters": lambda: cloud.clusters(cp, intr, image_size), "regions": lambda: cloud.regions(params, intr, image_size)}, reps)
    doc.update({k: summary(v) for k, v in ms.items()})
    ratio = np.asarray(ms["regions"]) / np.asarray(ms["clusters"])   # round by round: the two calls of a round ran back to back
    doc["regions_over_clusters"] = {"median": round(float(np.median(ratio)), 3), "p10": round(float(np.percentile(ratio, 10)), 3),
                                    "p90": round(float(np.percentile(ratio, 90)), 3)}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_region_timing.json"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("region_timing.py needs a GPU")
    doc = {"tool": "tools/region_timing.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps}
    from test_gpu_frame import _render_frame
    scene, depth, boxes, K, objs, solid = _render_frame(np.load(os.path.join(D.GOLDEN, "bottle_model_xyzn.npy")))
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    doc["rendered"] = stage(DeviceCloud.from_depth(depth, intr, fp64=True, normals={}), dict(tolerance=0.01, min_size=100), intr, depth.shape, a.reps)
    xyz, depth, _, intr = D.c1_frame()
    intr = tuple(float(v) for v in intr)
    kept = DeviceCloud.from_depth(depth, intr, fp64=True, normals={}).remove_planes(dict(n_hypotheses=256, max_planes=2))
    doc["c1"] = stage(kept, dict(tolerance=0.01, min_size=200), intr, depth.shape, a.reps)
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
