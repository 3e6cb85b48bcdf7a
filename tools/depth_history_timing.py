"""Time ppf_depth_history_push_device, the temporal step in front of the depth filter, against the filter.

Inputs:
  c1_frame   the reference's frame (tests/golden/c1_depth_window.npz, 720 x 1280 float32, 166,718 kept pixels)
  rendered   the two-bottle frame of tests/test_gpu_frame.py::_render_frame (360 x 640, every pixel kept)
Each is made a stream of 2 x 16 + 2 frames: seeded noise 0.001 z^2 and one kept pixel in ten dropped per frame, resident on
the device.  Routes, device entry to device entry on resident torch tensors, alternating in one process after one warm-up
(median and p10 - p90 of `--reps`, default 50; round r pushes frame r mod 34), per input:
  push_k4_median ... push_k16_mean   DepthHistory.push(tensor, out=tensor) at window 4, 8, 16, both modes, max_age window - 1
                                     ppf_depth_history_push_device
  filter_device_entry                filter_depth(tensor, out=tensor), the defaults: the yardstick, ppf_depth_filter_device
Before anything is timed every history is held to the numpy oracle's bytes and counts (tests/depth_history_oracle.py) on the
whole frame over window + 2 pushes, and then reset.  Writes profiles/r24_depth_history_timing.json (or --out).  Run it under a
time limit of its own, and the kernel trace as a run of its own:
  timeout -k 10 600 python tools/depth_history_timing.py
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -o depth_history -- python tools/depth_history_timing.py --reps 5 --no-write
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

import depth_history_oracle as H  # noqa: E402
import prep_data as D  # noqa: E402
from yolo_ppf_pose_estimation_amd import _capi  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DepthHistory, filter_depth  # noqa: E402

WINDOWS = (4, 8, 16)
N_FRAMES = 2 * 16 + 2
PARAMS = dict(range_abs=0.004, range_quad=0.004)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def stream(depth, seed):
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(N_FRAMES):
        z = depth + (0.001 * rng.standard_normal(depth.shape)).astype(np.float32) * depth * depth
        z[rng.random(depth.shape) < 0.1] = 0
        frames.append(np.ascontiguousarray(z, np.float32))
    return frames


def run_case(name, depth, reps, seed):
    import torch
    frames = stream(np.ascontiguousarray(depth, np.float32), seed)
    tensors = [torch.from_numpy(f).cuda() for f in frames]
    out = torch.empty_like(tensors[0])
    torch.cuda.synchronize()
    hists, routes, last = {}, {}, {}
    for window in WINDOWS:
        for mean in (False, True):
            key = f"push_k{window}_{'mean' if mean else 'median'}"
            prm = dict(PARAMS, window=window, max_age=window - 1, flags=_capi.PPF_HISTORY_MEAN if mean else 0)
            h = DepthHistory(depth.shape, params=prm)
            ora = H.History(window=window, max_age=window - 1, mean=mean, **PARAMS)
            for t in range(window + 2):       # the device is the oracle's bytes before anything is timed
                want = ora.push(frames[t])
                got, state, st = h.push(tensors[t], out=out, return_state=True, return_stats=True)
                assert got.cpu().numpy().tobytes() == want[0].tobytes() and state.cpu().numpy().tobytes() == want[1].tobytes(), (name, key, t)
                assert {k: st[k] for k in H.COUNTS} == want[2], (name, key, t, st, want[2])
            h.reset()
            last[key] = want[2]
            hists[key] = h
            routes[key] = lambda r, h=h: h.push(tensors[r % N_FRAMES], out=out)
    routes["filter_device_entry"] = lambda r: filter_depth(tensors[r % N_FRAMES], out=out)
    for r in range(16):                        # the one warm-up: every ring full
        for fn in routes.values():
            fn(r)
    print(f"{name}: equal to the oracle; timing", file=sys.stderr, flush=True)
    ms = {k: [] for k in routes}
    for r in range(reps):
        for key, fn in routes.items():
            res, dt = timed(lambda: fn(16 + r))
            ms[key].append(dt)
            del res
    res = {"case": name, "shape": list(depth.shape), "equal_to_oracle": True, "params": PARAMS,
           "counts_after_window_plus_2": last["push_k8_median"]}
    base = np.asarray(ms["filter_device_entry"])
    for key, v in ms.items():
        v = np.asarray(v)
        res[key] = {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
                    "p90_ms": round(float(np.percentile(v, 90)), 4), "reps": int(v.size)}
        if key != "filter_device_entry":
            ratio = v / base                   # round by round: both routes ran back to back
            res[key]["over_filter_median"] = round(float(np.median(ratio)), 3)
            res[key]["over_filter_p10_p90"] = [round(float(np.percentile(ratio, 10)), 3), round(float(np.percentile(ratio, 90)), 3)]
            res[key]["device_bytes"] = hists[key].info()["device_bytes"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_depth_history_timing.json"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_history_timing.py needs a GPU")
    from test_gpu_frame import _render_frame
    _, depth, _, _ = D.c1_frame()
    bottle = np.load(os.path.join(ROOT, "tests", "golden", "bottle_model_xyzn.npy"))
    _, rdepth, _, _, _, _ = _render_frame(bottle)
    cases = [run_case("c1_frame", depth, a.reps, 24), run_case("rendered", np.ascontiguousarray(rdepth, np.float32), a.reps, 25)]
    doc = {"tool": "tools/depth_history_timing.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": cases}
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
