"""What tools/verify_timing.py, render_timing.py and select_timing.py share: the three cases on the frame chain's own inputs
and the command line.  Each tool passes its own ``run_case(name, dets, poses, depth, intr, reps)``, which times its calls
on one case and returns the case's JSON record.

Cases (top 5):
  c1_k1 / c1_k8  the golden C1 chain's five ICP poses (tests/golden/c1_pipeline_golden.npz) of the bottle model (19,753 rows)
                 against the C1 object cloud of ppf_prep_frame, one detection or eight copies of it; C1 depth frame 720 x 1280
  rendered       the rendered two-bottle-and-box frame (tests/test_gpu_frame.py::_render_frame, 360 x 640): the refined top
                 poses ppf_match_frame returns for its three detections
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import prep_data as D  # noqa: E402
from yolo_ppf_pose_estimation_amd._capi import FrameDetection, IcpParams, MatchFrameStats, Pose, check, lib  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud  # noqa: E402
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector  # noqa: E402

PREP = dict(leaf=0.003, mean_k=50, stddev_mul=1.0, normal_k=30, curvature_threshold=0.03)


def stats(v):
    v = np.asarray(v)
    return {"median_ms": round(float(np.median(v)), 4), "p10_ms": round(float(np.percentile(v, 10)), 4),
            "p90_ms": round(float(np.percentile(v, 90)), 4)}


def c1_cases(bottle, reps, run_case):
    xyz, depth, box, intr = D.c1_frame()
    obj = DeviceCloud.upload(xyz).prep_frame([box], depth, intr, PREP)[0][0]
    golden = np.load(os.path.join(ROOT, "tests", "golden", "c1_pipeline_golden.npz"))
    poses = [golden["icp_poses"][k] for k in range(5)]
    mc = DeviceCloud.upload(bottle)
    out = [run_case(f"c1_k{K}", [(mc, obj)] * K, [poses] * K, depth, intr, reps) for K in (1, 8)]
    out[0]["model_rows"], out[0]["object_rows"] = int(bottle.shape[0]), len(obj)
    return out


def rendered_case(bottle, reps, run_case):
    from test_gpu_frame import _render_frame
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    pairs = DeviceCloud.upload(scene).prep_frame(boxes, depth, intr, dict(PREP, leaf=0.004))
    det_b = PPF3DDetector(0.05, 0.05).trainModel(bottle)
    det_s = PPF3DDetector(0.05, 0.05).trainModel(solid)
    mcs = [DeviceCloud.upload(bottle), DeviceCloud.upload(bottle), DeviceCloud.upload(solid)]
    fd = (FrameDetection * 3)()
    for i, d in enumerate((det_b, det_b, det_s)):
        fd[i].model, fd[i].model_cloud, fd[i].scene, fd[i].edge = d._model.ptr, mcs[i]._ptr, pairs[i][0]._ptr, pairs[i][1]._ptr
    ip = IcpParams()
    lib().ppf_default_icp_params(C.byref(ip))
    out, n_out = (Pose * 15)(), (C.c_int * 3)()
    check(lib().ppf_match_frame(fd, 3, C.byref(det_b._params(0.05, 0.05, False)), C.byref(ip), 5, out, n_out, None,
                                C.byref(MatchFrameStats())))
    poses = [[np.array(out[i * 5 + k].pose).reshape(4, 4) for k in range(n_out[i])] for i in range(3)]
    return run_case("rendered", [(mcs[i], pairs[i][0]) for i in range(3)], poses, depth, intr, reps)


def main(tool, profile, run_case):
    """the command line of a timing tool: the three cases through ``run_case``, printed and written to profiles/<profile>"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", profile))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} needs a GPU")
    bottle = np.load(os.path.join(ROOT, "tests", "golden", "bottle_model_xyzn.npy"))
    cases = c1_cases(bottle, a.reps, run_case) + [rendered_case(bottle, a.reps, run_case)]
    doc = {"tool": f"tools/{tool}", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cases": cases}
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
