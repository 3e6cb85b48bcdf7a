"""Time ppf_refine_frame against the verification calls that move and project the same model rows once, on the frame
chain's own inputs.

Cases (default refine, verify and render parameters, top 5):
  c1_k1 / c1_k8  the golden C1 chain's five ICP poses (tests/golden/c1_pipeline_golden.npz) of the bottle model (19,753 rows)
                 against the C1 object cloud of ppf_prep_frame, one detection or eight copies of it; C1 depth frame 720 x 1280
  rendered       the rendered two-bottle-and-box frame (tests/test_gpu_frame.py::_render_frame, 360 x 640): the refined top
                 poses ppf_match_frame returns for its three detections
Per case: the median and spread of the wall time of each call (perf_counter around the wrapper; `--reps` rounds after a
warm-up, each round calling ppf_verify_frame with the depth image, ppf_verify_frame_rendered and ppf_refine_frame,
alternating), the call's own ms_wall, its launches and host synchronisations, the ratio of refine's median to each
verification's, and refine's iterations and status per job.  Writes profiles/r14_refine_timing.json (or --out).
The kernel trace is a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o refine -- python tools/refine_timing.py --reps 5 --no-write
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_cases  # noqa: E402
from frame_cases import stats  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import refine_frame, verify_frame, verify_frame_rendered  # noqa: E402


def run_case(name, dets, poses, depth, intr, reps):
    res = {"case": name, "detections": len(dets), "poses": sum(len(p) for p in poses), "depth_shape": list(depth.shape), "reps": reps}
    mclouds = [d[0] for d in dets]
    info = refine_frame(mclouds, poses, depth, intr, top=5)[1]
    live = info["status"] != 0
    res["refine_iterations"] = [int(v) for v in info["iterations"][live]]
    res["refine_status"] = [int(v) for v in info["status"][live]]
    res["refine_rmse_first_mm"] = [round(float(v) * 1e3, 4) for v in info["rmse_first"][live]]
    res["refine_rmse_last_mm"] = [round(float(v) * 1e3, 4) for v in info["rmse_last"][live]]
    routes = {"verify_with_depth": lambda: verify_frame(dets, poses, 5, depth, intr)[2],
              "rendered_with_depth": lambda: verify_frame_rendered(dets, poses, 5, depth, intr)[2],
              "refine": lambda: refine_frame(mclouds, poses, depth, intr, top=5, return_stats=True)[2]}
    for fn in routes.values():   # warm-up
        fn()
        fn()
    wall = {k: [] for k in routes}
    call = {k: [] for k in routes}
    counters = {}
    for _ in range(reps):
        for key, fn in routes.items():
            t0 = time.perf_counter()
            st = fn()
            wall[key].append((time.perf_counter() - t0) * 1e3)
            call[key].append(st["ms_wall"])
            counters[key] = {k: st[k] for k in ("n_launches", "n_host_syncs", "n_jobs") if k in st}
    for key in wall:
        res[key] = dict(wall=stats(wall[key]), call_ms_wall=stats(call[key]), **counters[key])
    for key in ("verify_with_depth", "rendered_with_depth"):
        res[f"refine_over_{key}"] = round(res["refine"]["wall"]["median_ms"] / res[key]["wall"]["median_ms"], 3)
    return res


if __name__ == "__main__":
    frame_cases.main("refine_timing.py", "r14_refine_timing.json", run_case)
