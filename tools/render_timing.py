"""Time self-occlusion-aware pose verification (ppf_verify_frame_rendered) against ppf_verify_frame, and ppf_render_frame
of the best poses, on the frame chain's own inputs.

Cases, each with and without the depth image (default verify and render parameters, top 5):
  c1_k1 / c1_k8  the golden C1 chain's five ICP poses (tests/golden/c1_pipeline_golden.npz) of the bottle model (19,753 rows)
                 against the C1 object cloud of ppf_prep_frame, one detection or eight copies of it; C1 depth frame 720 x 1280
  rendered       the rendered two-bottle-and-box frame (tests/test_gpu_frame.py::_render_frame, 360 x 640): the refined top
                 poses ppf_match_frame returns for its three detections
Per case: the median and spread of the wall time of each call (perf_counter around the wrapper; `--reps` rounds, each
round calling ppf_verify_frame and ppf_verify_frame_rendered with and without depth, alternating, then ppf_render_frame of
the rendered entry's best poses at the image's size), the call's own ms_wall, its launches and host synchronisations.  Writes profiles/r10_render_timing.json (or --out).
The kernel trace is a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o render -- python tools/render_timing.py --reps 5 --no-write
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_cases  # noqa: E402
from frame_cases import stats  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import render_frame, verify_frame, verify_frame_rendered  # noqa: E402


def run_case(name, dets, poses, depth, intr, reps):
    res = {"case": name, "detections": len(dets), "poses": sum(len(p) for p in poses), "depth_shape": list(depth.shape), "reps": reps}
    shape = depth.shape
    routes = {"verify_cloud_only": lambda: verify_frame(dets, poses, 5, None, None),
              "rendered_cloud_only": lambda: verify_frame_rendered(dets, poses, 5, None, intr, image_size=shape),
              "verify_with_depth": lambda: verify_frame(dets, poses, 5, depth, intr),
              "rendered_with_depth": lambda: verify_frame_rendered(dets, poses, 5, depth, intr)}
    for fn in routes.values():   # warm-up
        fn()
    best = [int(b) for b in verify_frame_rendered(dets, poses, 5, depth, intr)[1]]
    mclouds = [d[0] for d in dets]

    def render():
        return render_frame(mclouds, poses, best, shape[0], shape[1], intr, return_stats=True)[2]

    render()
    wall = {k: [] for k in list(routes) + ["render_frame"]}
    call = {k: [] for k in wall}
    counters = {}
    for _ in range(reps):
        for key, fn in list(routes.items()) + [("render_frame", None)]:
            t0 = time.perf_counter()
            st = fn()[2] if fn else render()
            wall[key].append((time.perf_counter() - t0) * 1e3)
            call[key].append(st["ms_wall"])
            counters[key] = {"n_launches": st["n_launches"], "n_host_syncs": st["n_host_syncs"], "n_jobs": st["n_jobs"]}
    for key in wall:
        res[key] = dict(wall=stats(wall[key]), call_ms_wall=stats(call[key]), **counters[key])
    for d in ("cloud_only", "with_depth"):
        res[f"rendered_over_verify_{d}"] = round(res[f"rendered_{d}"]["wall"]["median_ms"] / res[f"verify_{d}"]["wall"]["median_ms"], 3)
    res["best"] = best
    return res


if __name__ == "__main__":
    frame_cases.main("render_timing.py", "r10_render_timing.json", run_case)
