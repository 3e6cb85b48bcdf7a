"""Time ppf_depth_segments against ppf_prep_regions / ppf_prep_clusters, the stages it stands beside, on the same frame.

Inputs, both filtered (ppf_depth_filter at its defaults) and with the normals of ppf_cloud_from_depth_normals at its defaults:
  rendered  the two-bottle frame of tests/test_gpu_frame.py::_render_frame (360 x 640), background and all
  c1        the reference's frame (tests/golden/c1_depth_window.npz, 720 x 1280; the pixels outside its window are empty)
Routes, alternating in one process after a warm-up (median and spread of `--reps`), per input, every parameter at its default:
  regions          cloud.regions(intr, image size)                    ppf_prep_regions on the frame's cloud: the yardstick
  segments         segment_depth(resident tensor, normals=cloud)      ppf_depth_segments_device
  clusters         cloud.clusters(intr, image size)                   ppf_prep_clusters on the same cloud
  segments_depth   segment_depth(resident tensor)                     the same without normals
The device is held to the oracles on both inputs (segments with and without normals: labels, info, counts, pixel counts;
regions: info, counts, labels) before anything is timed.  Writes the next free profiles/rNN_depth_segments_timing.json (or
--out).  The kernel trace is a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o segments -- python tools/depth_segments_timing.py --reps 5 --no-write
"""
import argparse
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import depth_segments_oracle as S  # noqa: E402
import prep_data as D  # noqa: E402
import region_oracle as R  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud, filter_depth, segment_depth  # noqa: E402


def summary(v):
    v = np.asarray(v)
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
            "p90_ms": round(float(np.percentile(v, 90)), 4)}


def ratio(a, b):
    r = np.asarray(a) / np.asarray(b)   # round by round: the calls of a round ran back to back
    return {"median": round(float(np.median(r)), 3), "p10": round(float(np.percentile(r, 10)), 3), "p90": round(float(np.percentile(r, 90)), 3)}


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


def held_to_the_oracle(t, filtered, normals, cloud):
    got = segment_depth(t, normals=cloud, return_info=True, return_stats=True)
    want = S.segments(filtered, normals=normals)
    same = (got[0].cpu().numpy().tobytes() == want[0].tobytes() and tuple(int(c) for c in got[2]) == want[2]
            and all(got[3][k] == v for k, v in want[3].items())
            and [int(r["n_pixels"]) for r in got[1]] == [i["n_pixels"] for i in want[1]]
            and [tuple(int(v) for v in r["box_xywh"]) for r in got[1]] == [i["box_xywh"] for i in want[1]])
    assert same, "segments: the device differs from the oracle"
    return got


def stage(depth, intr, reps):
    import torch
    t = filter_depth(torch.from_numpy(np.ascontiguousarray(depth, np.float32)).cuda())
    filtered = t.cpu().numpy()
    cloud = DeviceCloud.from_depth(t, intr, fp64=True, normals={})
    rows, curv = cloud.download()
    labels, info, counts, stats = held_to_the_oracle(t, filtered, (rows, curv), cloud)
    _, dinfo, dcounts, dstats = held_to_the_oracle(t, filtered, None, None)
    _, rinfo, rcounts, rlabels, rstats = cloud.regions(None, intr, depth.shape, return_info=True, return_labels=True)
    want = R.regions(rows, None, curv, intr, depth.shape)
    assert rinfo.tobytes() == want[1].tobytes() and (rcounts == want[2]).all() and (rlabels == want[3]).all(), "regions: the device differs from the oracle"
    _, cinfo, ccounts, cstats = cloud.clusters(None, intr, depth.shape, return_info=True)
    doc = {"image": list(depth.shape), "params": dict(S.DEFAULTS), "pixel_counts": {k: v for k, v in stats.items() if k.startswith("n_")},
           "counts": [int(v) for v in counts], "segment_pixels": [int(v) for v in info["n_pixels"]],
           "depth_only_counts": [int(v) for v in dcounts], "depth_only_launches": dstats["n_launches"],
           "region_counts": [int(v) for v in rcounts], "region_rows": [int(v) for v in rinfo["n_rows"][:int(rcounts[0])]],
           "region_counters": {k: v for k, v in rstats.items() if k.startswith("n_")},
           "cluster_counts": [int(v) for v in ccounts], "cluster_counters": {k: v for k, v in cstats.items() if k.startswith("n_")}}
    ms = alternate({"regions": lambda: cloud.regions(None, intr, depth.shape), "segments": lambda: segment_depth(t, normals=cloud),
                    "clusters": lambda: cloud.clusters(None, intr, depth.shape), "segments_depth": lambda: segment_depth(t)}, reps)
    doc.update({k: summary(v) for k, v in ms.items()})
    doc["segments_over_regions"] = ratio(ms["segments"], ms["regions"])
    doc["segments_depth_over_clusters"] = ratio(ms["segments_depth"], ms["clusters"])
    return doc


def next_free():
    taken = [int(m.group(1)) for m in (re.match(r"r(\d+)_", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*"))) if m]
    return os.path.join(ROOT, "profiles", f"r{max(taken + [0]) + 1:02d}_depth_segments_timing.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_segments_timing.py needs a GPU")
    doc = {"tool": "tools/depth_segments_timing.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps}
    from test_gpu_frame import _render_frame
    _, depth, _, K, _, _ = _render_frame(np.load(os.path.join(D.GOLDEN, "bottle_model_xyzn.npy")))
    doc["rendered"] = stage(depth, (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])), a.reps)
    _, depth, _, intr = D.c1_frame()
    doc["c1"] = stage(depth, tuple(float(v) for v in intr), a.reps)
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out or next_free(), "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
