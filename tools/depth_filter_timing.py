"""Time ppf_depth_filter, the step in front of the scene cloud, against the step it precedes.

Inputs:
  c1_frame   the reference's frame (tests/golden/c1_depth_window.npz, 720 x 1280 float32, 166,718 kept pixels)
  rendered   the two-bottle frame of tests/test_gpu_frame.py::_render_frame (360 x 640, every pixel kept)
Routes, device entry to device entry on a resident torch tensor, alternating in one process after one warm-up (median and
p10 - p90 of `--reps`, default 50), per input:
  filter_device_entry    filter_depth(tensor, out=tensor), the defaults (radius 3)        ppf_depth_filter_device
  normals_device_entry   DeviceCloud.from_depth(tensor, normals=dict(radius=3))           ppf_cloud_from_depth_normals_device,
                         the yardstick: the same window walked twice, with a Jacobi solve per pixel and a compaction
Before anything is timed the filter is held to the numpy oracle's bytes and counts (tests/depth_filter_oracle.py) on the
whole frame.  Writes profiles/r20_depth_filter_timing.json (or --out).  Run it under a time limit of its own, and the kernel
trace as a run of its own:
  timeout -k 10 300 python tools/depth_filter_timing.py
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d <dir> -o depth_filter -- python tools/depth_filter_timing.py --reps 5 --no-write
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

import depth_filter_oracle as F  # noqa: E402
import prep_data as D  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud, filter_depth  # noqa: E402

RADIUS = 3


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
    out = torch.empty_like(t)
    torch.cuda.synchronize()
    routes = {
        "filter_device_entry": lambda: filter_depth(t, out=out),
        "normals_device_entry": lambda: DeviceCloud.from_depth(t, intr, fp64=True, normals=dict(radius=RADIUS)),
    }
    want, counts = F.filter_depth(depth)
    got, st = filter_depth(t, out=out, return_stats=True)       # the device is the oracle's bytes before anything is timed
    assert got.cpu().numpy().tobytes() == want.tobytes() and {k: st[k] for k in counts} == counts, (name, st, counts)
    for fn in routes.values():                                 # the one warm-up
        fn()
    print(f"{name}: {counts}, equal to the oracle; timing", file=sys.stderr, flush=True)
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for key, fn in routes.items():
            res, dt = timed(fn)
            ms[key].append(dt)
            del res
    res = {"case": name, "shape": list(depth.shape), "radius": RADIUS, "equal_to_oracle": True}
    res.update(counts)
    for key, v in ms.items():
        v = np.asarray(v)
        res[key] = {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                    "p90_ms": round(float(np.percentile(v, 90)), 4), "reps": int(v.size)}
    res["filter_over_normals"] = round(res["filter_device_entry"]["median_ms"] / res["normals_device_entry"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_depth_filter_timing.json"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_filter_timing.py needs a GPU")
    from test_gpu_frame import _render_frame
    _, depth, _, intr = D.c1_frame()
    bottle = np.load(os.path.join(ROOT, "tests", "golden", "bottle_model_xyzn.npy"))
    _, rdepth, _, K, _, _ = _render_frame(bottle)
    cases = [run_case("c1_frame", depth, intr, a.reps),
             run_case("rendered", np.ascontiguousarray(rdepth, np.float32), (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), a.reps)]
    doc = {"tool": "tools/depth_filter_timing.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": cases}
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
