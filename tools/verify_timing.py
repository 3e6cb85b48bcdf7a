"""Time pose verification (ppf_verify_frame) on the frame chain's own inputs.

Cases, each with and without the depth image (default parameters, top 5):
  c1_k1 / c1_k8  the golden C1 chain's five ICP poses (tests/golden/c1_pipeline_golden.npz) of the bottle model (19,753 rows)
                 against the C1 object cloud of ppf_prep_frame, one detection or eight copies of it; C1 depth frame 720 x 1280
  rendered       the rendered two-bottle-and-box frame (tests/test_gpu_frame.py::_render_frame, 360 x 640): the refined top
                 poses ppf_match_frame returns for its three detections
Per case: the median and spread of the wall time of the call (perf_counter around verify_frame, `--reps` calls alternating
with and without depth), the call's own ms_wall, its launches and host synchronisations.  `depth_upload_ms` is a plain
host-to-device copy of the same image (torch, pageable memory), the part of the depth run that is the upload.  Writes
profiles/r09_verify_timing.json (or --out).  The kernel trace is a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o verify -- python tools/verify_timing.py --reps 5 --no-write
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_cases  # noqa: E402
from frame_cases import stats  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import verify_frame  # noqa: E402


def upload_ms(depth, reps):
    import torch
    v = []
    for _ in range(reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = torch.from_numpy(depth).cuda()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
        del t
    return stats(v[3:])


def run_case(name, dets, poses, depth, intr, reps):
    res = {"case": name, "detections": len(dets), "poses": sum(len(p) for p in poses), "depth_shape": list(depth.shape),
           "depth_bytes": int(depth.nbytes), "reps": reps}
    routes = {"cloud_only": (None, None), "with_depth": (depth, intr)}
    for key, (d, it) in routes.items():   # warm-up
        verify_frame(dets, poses, 5, d, it)
    wall = {k: [] for k in routes}
    call = {k: [] for k in routes}
    counters = {}
    for _ in range(reps):
        for key, (d, it) in routes.items():
            t0 = time.perf_counter()
            _, best, st = verify_frame(dets, poses, 5, d, it)
            wall[key].append((time.perf_counter() - t0) * 1e3)
            call[key].append(st["ms_wall"])
            counters[key] = {"n_launches": st["n_launches"], "n_host_syncs": st["n_host_syncs"], "n_jobs": st["n_jobs"],
                             "best": [int(b) for b in best]}
    for key in routes:
        res[key] = dict(wall=stats(wall[key]), call_ms_wall=stats(call[key]), **counters[key])
    res["depth_extra_ms"] = round(res["with_depth"]["wall"]["median_ms"] - res["cloud_only"]["wall"]["median_ms"], 4)
    res["depth_upload_ms"] = upload_ms(depth, reps)
    return res


if __name__ == "__main__":
    frame_cases.main("verify_timing.py", "r09_verify_timing.json", run_case)
