"""Time match + ICP of a frame with K detections: the per-detection loop against one ppf_match_frame call.

Cases: K = 1, 2, 4, 8, 16 copies of the C1 detection (tests/golden/c1_depth_window.npz, its box, the bottle model,
trainModel(0.025, 0.05), match_S2B(0.05, 0.05), top 5, ICP(100, 0.005, 2.5, 8)), then the rendered three-object,
two-model frame of tests/test_gpu_frame.py.  The clouds are prepared once (ppf_prep_frame); each case is warmed up, then
the two routes alternate in the same process (median of `--reps`) and their outputs are checked equal bit for bit.
Writes profiles/r06_match_frame_timing.json.  The kernel trace is a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o match_frame -- python tools/match_frame_timing.py --reps 3 --no-write
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import prep_data as D  # noqa: E402
from yolo_ppf_pose_estimation_amd._capi import FrameDetection, IcpParams, MatchFrameStats, Pose, check, lib  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud  # noqa: E402
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector  # noqa: E402

P = dict(leaf=0.003, mean_k=50, stddev_mul=1.0, normal_k=30, curvature_threshold=0.03)
TOP = 5


def icp_params():
    p = IcpParams()
    lib().ppf_default_icp_params(C.byref(p))
    return p


def loop(entries, mp, ip):
    """ppf_match_clouds + ppf_icp_refine_clouds per detection: (rows, ms match, ms ICP)"""
    rows, tm, ti = [], 0.0, 0.0
    for det, mc, obj, edge in entries:
        cap = len(obj) + 8
        out, n = (Pose * cap)(), C.c_int(0)
        t0 = time.perf_counter()
        check(lib().ppf_match_clouds(det._model.ptr, obj._ptr, edge._ptr, C.byref(mp), out, cap, C.byref(n)))
        t1 = time.perf_counter()
        k = min(TOP, n.value)
        if k:
            check(lib().ppf_icp_refine_clouds(mc._ptr, obj._ptr, C.byref(ip), out, k, None))
        t2 = time.perf_counter()
        tm += t1 - t0
        ti += t2 - t1
        rows.append([bytes(out[i]) for i in range(k)])
    return rows, tm * 1e3, ti * 1e3


def one_pass(entries, mp, ip):
    n = len(entries)
    dets = (FrameDetection * n)()
    for i, (det, mc, obj, edge) in enumerate(entries):
        dets[i].model, dets[i].model_cloud, dets[i].scene, dets[i].edge = det._model.ptr, mc._ptr, obj._ptr, edge._ptr
    out, n_out, st = (Pose * (n * TOP))(), (C.c_int * n)(), MatchFrameStats()
    check(lib().ppf_match_frame(dets, n, C.byref(mp), C.byref(ip), TOP, out, n_out, None, C.byref(st)))
    return [[bytes(out[i * TOP + k]) for k in range(n_out[i])] for i in range(n)], st


def run_case(name, entries, mp, ip, reps):
    for _ in range(3):   # warm-up: contexts, block cache, code objects
        loop(entries, mp, ip)
        one_pass(entries, mp, ip)
    tl, tlm, tli, tf, tfm, tfi = [], [], [], [], [], []
    same = True
    for _ in range(reps):
        t0 = time.perf_counter()
        lr, lm, li = loop(entries, mp, ip)
        tl.append((time.perf_counter() - t0) * 1e3)
        tlm.append(lm)
        tli.append(li)
        t0 = time.perf_counter()
        fr, st = one_pass(entries, mp, ip)
        tf.append((time.perf_counter() - t0) * 1e3)
        tfm.append(st.ms_match)
        tfi.append(st.ms_icp)
        same &= lr == fr
    med = lambda v: float(np.median(v))  # noqa: E731
    row = {"case": name, "K": len(entries), "loop_ms": med(tl), "loop_match_ms": med(tlm), "loop_icp_ms": med(tli),
           "frame_ms": med(tf), "frame_match_ms": med(tfm), "frame_icp_ms": med(tfi), "speedup": med(tl) / med(tf),
           "icp_speedup": med(tli) / med(tfi), "frame_n_icp_jobs": st.n_icp_jobs, "frame_n_icp_launches": st.n_icp_launches,
           "frame_n_icp_passes": st.n_icp_passes, "frame_n_host_syncs": st.n_host_syncs, "identical": bool(same)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_match_frame_timing.json"))
    a = ap.parse_args()
    bottle = np.load(os.path.join(ROOT, "tests", "golden", "bottle_model_xyzn.npy"))
    ip = icp_params()
    res = {"top": TOP, "reps": a.reps, "cases": []}
    # C1: the golden frame and box, K copies of the detection
    xyz, depth, box, intr = D.c1_frame()
    pairs = DeviceCloud.upload(xyz).prep_frame([box], depth, intr, P)
    det = PPF3DDetector(0.025, 0.05).trainModel(bottle)
    mc = DeviceCloud.upload(bottle)
    mp = det._params(0.05, 0.05, False)
    for k in (1, 2, 4, 8, 16):
        res["cases"].append(run_case(f"c1_x{k}", [(det, mc, pairs[0][0], pairs[0][1])] * k, mp, ip, a.reps))
    # the rendered frame: two bottles and a box, two models of different sizes
    from test_gpu_frame import _render_frame
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    pairs = DeviceCloud.upload(scene).prep_frame(boxes, depth, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), dict(P, leaf=0.004))
    db = PPF3DDetector(0.05, 0.05).trainModel(bottle)
    ds = PPF3DDetector(0.05, 0.05).trainModel(solid)
    cs = DeviceCloud.upload(solid)
    entries = [(db, mc, pairs[0][0], pairs[0][1]), (db, mc, pairs[1][0], pairs[1][1]), (ds, cs, pairs[2][0], pairs[2][1])]
    res["cases"].append(run_case("rendered_3obj_2models", entries, db._params(0.05, 0.05, False), ip, a.reps))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
