"""Time ppf_depth_edges on the reference's frame against its two sibling stages on the depth image.

Input: c1_frame, the reference's frame (tests/golden/c1_depth_window.npz, 720 x 1280 float32, 166,718 kept pixels).
Routes, device entry to device entry on a resident torch tensor, alternating in one process after one warm-up (median and
p10 - p90 of `--reps`, default 50):
  edges_mask             depth_edges(tensor, out=tensor)                                   one launch, one wait
  edges_normals          depth_edges(tensor, normals=cloud, out=tensor)                    7 launches, one wait
  edges_normals_cloud    depth_edges(tensor, normals=cloud, out=tensor, cloud=True)        13 launches, two waits
  edges_cloud            depth_edges(tensor, intr, out=tensor, cloud=True)                 7 launches, two waits
  filter_device_entry    filter_depth(tensor, out=tensor), the defaults                    ppf_depth_filter_device
  segments_device_entry  segment_depth(tensor, out=tensor), no normals                     ppf_depth_segments_device
Beside each edges route stands the time its streamed bytes take at 6.3 TB/s (the image and the mask once per pass that
touches them, the normals rows that are read, the cloud rows that are written): the floor the route cannot go below.
Before anything is timed the mask, the counts and the cloud are held to the numpy oracle's bytes (tests/depth_edges_oracle.py)
on the whole frame, with the device's own normals cloud.  Writes profiles/r36_depth_edges_timing.json (or --out).  Run it
under a time limit of its own:
  timeout -k 10 300 python tools/depth_edges_timing.py
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

import depth_edges_oracle as E  # noqa: E402
import prep_data as D  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud, depth_edges, filter_depth, segment_depth  # noqa: E402

HBM_BYTES_PER_MS = 6.3e9


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def run_case(name, depth, intr, reps):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).cuda()
    mask = torch.empty(t.shape, dtype=torch.uint8, device="cuda")
    fout = torch.empty_like(t)
    labels = torch.empty(t.shape, dtype=torch.int32, device="cuda")
    scene = DeviceCloud.from_depth(t, intr, fp64=True, normals={})
    torch.cuda.synchronize()
    routes = {
        "edges_mask": lambda: depth_edges(t, out=mask),
        "edges_normals": lambda: depth_edges(t, normals=scene, out=mask),
        "edges_normals_cloud": lambda: depth_edges(t, normals=scene, out=mask, cloud=True),
        "edges_cloud": lambda: depth_edges(t, intr, fp64=True, out=mask, cloud=True),
        "filter_device_entry": lambda: filter_depth(t, out=fout),
        "segments_device_entry": lambda: segment_depth(t, out=labels),
    }
    # the device is the oracle's bytes before anything is timed
    nrm = scene.download()
    want = E.edges(depth, normals=nrm)
    got, edge, st = depth_edges(t, normals=scene, out=mask, cloud=True, return_stats=True)
    assert got.cpu().numpy().tobytes() == want[0].tobytes() and {k: st[k] for k in E.STAT_KEYS} == want[2], (name, st, want[2])
    rows, curv = edge.download()
    assert rows.tobytes() == want[1][0].tobytes() and curv.tobytes() == want[1][1].tobytes()
    plain = E.edges(depth, intr, fp64=True)
    got, edge, pst = depth_edges(t, intr, fp64=True, out=mask, cloud=True, return_stats=True)
    assert got.cpu().numpy().tobytes() == plain[0].tobytes() and edge.download()[0].tobytes() == plain[1][0].tobytes()
    del edge
    for fn in routes.values():                                 # the one warm-up
        fn()
    print(f"{name}: {want[2]}, equal to the oracle; timing", file=sys.stderr, flush=True)
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for key, fn in routes.items():
            res, dt = timed(fn)
            ms[key].append(dt)
            del res
    n, n_kept = depth.size, want[2]["n_kept"]
    runs = depth.shape[0] * ((depth.shape[1] + 63) // 64)
    streamed = {                                               # bytes each route cannot avoid moving
        "edges_mask": 4 * n + n,
        "edges_normals": 4 * n + n + 8 * runs + n + 28 * n_kept + 2 * n,
        "edges_normals_cloud": 4 * n + n + 8 * runs + n + 28 * n_kept + 2 * n + 8 * runs + n + 56 * want[2]["n_rows"],
        "edges_cloud": 4 * n + n + 8 * runs + n + 32 * plain[2]["n_rows"],
    }
    res = {"case": name, "shape": list(depth.shape), "equal_to_oracle": True, "with_normals": want[2], "without_normals": plain[2]}
    for key, v in ms.items():
        v = np.asarray(v)
        res[key] = {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                    "p90_ms": round(float(np.percentile(v, 90)), 4), "reps": int(v.size)}
        if key in streamed:
            res[key]["streamed_bytes"] = int(streamed[key])
            res[key]["at_6_3_TB_s_ms"] = round(streamed[key] / HBM_BYTES_PER_MS, 5)
    res["launches_waits"] = {"edges_mask": [1, 1], "edges_normals": [7, 1], "edges_cloud": [pst["n_launches"], pst["n_host_syncs"]],
                             "edges_normals_cloud": [st["n_launches"], st["n_host_syncs"]]}
    res["mask_over_filter"] = round(res["edges_mask"]["median_ms"] / res["filter_device_entry"]["median_ms"], 3)
    res["mask_over_segments"] = round(res["edges_mask"]["median_ms"] / res["segments_device_entry"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r36_depth_edges_timing.json"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_edges_timing.py needs a GPU")
    _, depth, _, intr = D.c1_frame()
    cases = [run_case("c1_frame", depth, intr, a.reps)]
    doc = {"tool": "tools/depth_edges_timing.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": cases}
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
