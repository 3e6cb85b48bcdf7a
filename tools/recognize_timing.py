"""Time ppf_recognize_frame against the only other way to name a proposal: matching it against every model.

Inputs: the four models of tests/recognize_cases.py (box, cylinder, torus, bottle) trained at 0.05 of their diameter with 12-degree
bins, and 8 proposals, two seeded one-sided views a model, each cut to exactly 512 rows.
Routes, alternating in one process after a warm-up (median and spread of `--reps`, default 20), each timed by the ms_wall of
its own stats record:
  recognize   ppf_recognize_frame over the 8 proposals and the 4 models, every parameter at its default
  match_all   ppf_match_frame over the same 32 (proposal, model) detections with top = 1 (match + ICP of the best pose), scene
              sampling 0.05 / 0.05 as CloudProcessor.MatchFrame's defaults
The recogniser is held to the numpy oracle on the same inputs before anything is timed.  Writes the next free
profiles/rNN_recognize_timing.json (or --out).  The kernel trace is a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o rec -- python tools/recognize_timing.py --reps 5 --no-write
"""
import argparse
import ctypes as C
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import recognize_cases as K  # noqa: E402
import recognize_oracle as R  # noqa: E402
from yolo_ppf_pose_estimation_amd._capi import FrameDetection, IcpParams, MatchFrameStats, Pose, check, lib  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud, Recognizer  # noqa: E402
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector  # noqa: E402


def summary(v):
    v = np.asarray(v)
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
            "p90_ms": round(float(np.percentile(v, 90)), 4)}


def next_free():
    taken = [int(m.group(1)) for m in (re.match(r"r(\d+)_", os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*"))) if m]
    return os.path.join(ROOT, "profiles", f"r{max(taken + [0]) + 1:02d}_recognize_timing.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    if lib().ppf_device_count() < 1:
        raise SystemExit("recognize_timing.py needs a GPU")
    fulls = [K.solid(k) for k in K.KINDS]
    dets = [PPF3DDetector(0.05, 0.05).trainModel(f) for f in fulls]
    views = [K.thin(K.one_sided_view(fulls[i % 4], 500 + i), 512, seed=i) for i in range(8)]
    assert all(v.shape[0] == 512 for v in views)
    clouds = [DeviceCloud.upload(v) for v in views]
    rec = Recognizer(dets)

    ranked, n_used, counts, st = rec.recognize(clouds, return_counts=True, return_stats=True)
    want = R.recognize(views, [R.Model.from_detector(d) for d in dets])
    for i, w in enumerate(want):
        assert int(n_used[i]) == w["n_used"] == 512 and np.array_equal(counts[i], w["counts"]), "recognize: the device differs from the oracle"
        assert [int(m) for m in ranked[i]["model"]] == w["ranked"]
    doc = {"tool": "tools/recognize_timing.py", "reps": a.reps, "n_proposals": 8, "rows": 512, "n_models": 4,
           "models": [dict(kind=k, **rec.model_info(i)) for i, k in enumerate(K.KINDS)],
           "launches": st["n_launches"], "host_syncs": st["n_host_syncs"],
           "named_right": sum(int(ranked[i]["model"][0]) == i % 4 for i in range(8)),
           "scores": [[round(float(s), 4) for s in w["scores"][:, 2]] for w in want]}

    model_clouds = [DeviceCloud.upload(f) for f in fulls]
    n_dets = 32
    frame = (FrameDetection * n_dets)()
    for i in range(8):
        for m in range(4):
            d = frame[i * 4 + m]
            d.model, d.model_cloud, d.scene, d.edge = dets[m]._model.ptr, model_clouds[m]._ptr, clouds[i]._ptr, None
    mp = dets[0]._params(0.05, 0.05, False)
    icp = IcpParams()
    lib().ppf_default_icp_params(C.byref(icp))
    poses, n_out, mst = (Pose * n_dets)(), (C.c_int * n_dets)(), MatchFrameStats()

    def match_all():
        check(lib().ppf_match_frame(frame, n_dets, C.byref(mp), C.byref(icp), 1, poses, n_out, None, C.byref(mst)))
        return mst.ms_wall

    def recognize():
        return rec.recognize(clouds, return_stats=True)[1]["ms_wall"]

    routes = {"recognize": recognize, "match_all": match_all}
    for _ in range(3):
        for fn in routes.values():
            fn()
    ms = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, fn in routes.items():
            ms[k].append(fn())
    doc.update({k: summary(v) for k, v in ms.items()})
    r = np.asarray(ms["recognize"]) / np.asarray(ms["match_all"])   # round by round: the calls of a round ran back to back
    doc["recognize_over_match_all"] = {"median": round(float(np.median(r)), 4), "p10": round(float(np.percentile(r, 10)), 4),
                                       "p90": round(float(np.percentile(r, 90)), 4)}
    doc["match_all_matched"] = int(sum(1 for v in n_out if v > 0))
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out or next_free(), "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
