"""Time ppf_depth_motion against what the library could do for the same job before it: the previous frame's cloud with normals
(ppf_cloud_from_depth_normals) refined as a "model" from the identity pose by ppf_refine_frame on the current depth image.

Inputs: a pair of frames made from each existing frame by a seeded camera motion of 20 mm / 2 degrees -- the frame's kept pixels
back-projected, moved by T and drawn into the nearest pixel of a second image with a z-buffer (the holes this leaves stay):
  c1_frame   the reference's frame (tests/golden/c1_depth_window.npz, 720 x 1280 float32, 166,718 kept pixels)
  rendered   the two-bottle frame of tests/test_gpu_frame.py::_render_frame (360 x 640, every pixel kept)
Routes, alternating in one process after one warm-up (median and p10 - p90 of `--reps`, default 50), per input:
  motion_device_entry   depth_motion on two resident torch tensors, the defaults (3 levels, 10 + 5 + 4 evaluations)  ppf_depth_motion_device
  motion_host_entry     depth_motion on two numpy images: the same with the two uploads                              ppf_depth_motion
  refine_step1          DeviceCloud.from_depth(prev tensor, normals) + refine_frame of it at the identity on the current image,
                        max_iters = the 19 evaluations of the motion's budget, model_step 1, the other refine defaults
  refine_step4          the same at model_step 4: as many rows as level 1 has pixels
Before anything is timed both motion entries are held to the numpy oracle's bytes (tests/depth_motion_oracle.py): pose, level
rows, counts.  Every route's pose error against the true motion is recorded next to its time, and the share of the enqueued
evaluations that returned at the state word.  Writes profiles/r26_depth_motion_timing.json (or --out).  Run it under a time
limit of its own, and the kernel trace as a run of its own:
  timeout -k 10 600 python tools/depth_motion_timing.py
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d <dir> -o depth_motion -- python tools/depth_motion_timing.py --reps 5 --no-write
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

import depth_motion_cases as Cs  # noqa: E402
import depth_motion_oracle as O  # noqa: E402
import prep_data as D  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud, depth_motion, refine_frame  # noqa: E402

SEED, MM, DEG = 7, 20.0, 2.0
BUDGET = sum(O.DEFAULTS["iters"][:O.DEFAULTS["levels"]])


def warp(depth, intr, T):
    """the frame seen after the camera's motion T: every kept pixel moved and drawn into its nearest pixel, nearest depth wins"""
    fx, fy, ppx, ppy = intr
    v, u = np.nonzero(depth > 0)
    z = depth[v, u].astype(np.float64)
    p = np.stack([(u - ppx) * z / fx, (v - ppy) * z / fy, z], axis=1) @ T[:3, :3].T + T[:3, 3]
    ui, vi = np.rint(p[:, 0] * fx / p[:, 2] + ppx).astype(np.int64), np.rint(p[:, 1] * fy / p[:, 2] + ppy).astype(np.int64)
    ok = (p[:, 2] > 0) & (ui >= 0) & (ui < depth.shape[1]) & (vi >= 0) & (vi < depth.shape[0])
    out = np.full(depth.shape, np.inf)
    np.minimum.at(out, (vi[ok], ui[ok]), p[ok, 2])
    return np.where(np.isfinite(out), out, 0.0).astype(np.float32)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def summary(v):
    v = np.asarray(v)
    return {"median": round(float(np.median(v)), 4), "p10": round(float(np.percentile(v, 10)), 4), "p90": round(float(np.percentile(v, 90)), 4),
            "reps": int(v.size)}


def run_case(name, prev, intr, reps):
    import torch
    T_true = Cs.true_motion(SEED, MM, DEG)
    prev = np.ascontiguousarray(prev, np.float32)
    cur = warp(prev, intr, T_true)
    tp, tc = torch.from_numpy(prev).cuda(), torch.from_numpy(cur).cuda()
    level1 = (prev.shape[0] // 2) * (prev.shape[1] // 2)

    def refine(step):
        cloud = DeviceCloud.from_depth(tp, intr, fp64=True, normals=dict(radius=3))
        poses, info = refine_frame([cloud], [[np.eye(4)]], cur, intr, dict(max_iters=BUDGET, model_step=step))
        return poses[0][0].pose, info[0, 0]

    routes = {
        "motion_device_entry": lambda: depth_motion(tp, tc, intr, return_info=True, return_stats=True),
        "motion_host_entry": lambda: depth_motion(prev, cur, intr, return_info=True, return_stats=True),
        "refine_step1": lambda: refine(1),
        "refine_step4": lambda: refine(4),
    }
    # the device is the oracle's bytes before anything is timed
    Tw, rows, stw = O.motion(prev, cur, intr)
    for key in ("motion_device_entry", "motion_host_entry"):
        T, info, st = routes[key]()
        assert T.tobytes() == Tw.tobytes() and all(st[k] == stw[k] for k in ("status", "n_evaluations", "n_enqueued", "n_launches")), (name, key)
        assert all(np.asarray(info[l][f]).tobytes() == np.asarray(rows[l][f], dtype=info.dtype[f]).tobytes() for l in range(4) for f in O.ROW_FIELDS)
    res = {"case": name, "shape": list(prev.shape), "kept_prev": int((prev > 0).sum()), "kept_cur": int((cur > 0).sum()), "level1_pixels": level1,
           "motion_mm": MM, "motion_deg": DEG, "seed": SEED, "equal_to_oracle": True, "budget": BUDGET}
    mm, deg = O.pose_error(Tw, T_true)
    res["motion"] = {"status": O.STATUS[stw["status"]], "error_mm": round(mm, 4), "error_deg": round(deg, 5), "n_launches": stw["n_launches"],
                     "n_evaluations": stw["n_evaluations"], "n_enqueued": stw["n_enqueued"],
                     "empty_share": round(1.0 - stw["n_evaluations"] / stw["n_enqueued"], 4),
                     "levels": [{k: (float(r[k]) if k.startswith("rmse") else int(r[k])) for k in O.ROW_FIELDS} for r in rows[:3]]}
    for step in (1, 4):
        T, row = refine(step)
        mm, deg = O.pose_error(T, T_true)
        res[f"refine_step{step}_result"] = {"status": int(row["status"]), "iterations": int(row["iterations"]), "n_rows": int(row["n_rows"]),
                                            "n_pairs_last": int(row["n_pairs_last"]), "error_mm": round(mm, 4), "error_deg": round(deg, 5)}
    print(f"{name}: equal to the oracle; {res['motion']}; timing", file=sys.stderr, flush=True)
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for key, fn in routes.items():
            out, dt = timed(fn)
            ms[key].append(dt)
            del out
    for key, v in ms.items():
        res[key + "_ms"] = summary(v)
    for key in ("refine_step1", "refine_step4", "motion_host_entry"):
        res[f"{key}_over_motion_device_entry"] = summary(np.asarray(ms[key]) / np.asarray(ms["motion_device_entry"]))   # round by round
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_depth_motion_timing.json"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("depth_motion_timing.py needs a GPU")
    from test_gpu_frame import _render_frame
    _, depth, _, intr = D.c1_frame()
    bottle = np.load(os.path.join(ROOT, "tests", "golden", "bottle_model_xyzn.npy"))
    _, rdepth, _, K, _, _ = _render_frame(bottle)
    cases = [run_case("c1_frame", depth, intr, a.reps),
             run_case("rendered", rdepth, (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])), a.reps)]
    doc = {"tool": "tools/depth_motion_timing.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": cases}
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
