#!/usr/bin/env python3
"""Non-zero columns of the count tables a workload's entries meet, from a diagnostic build of the library:

    tools/build_variant.sh diag -DPPF_DIAG_COLUMNS
    PPF_HIP_LIB=build_var/diag.so python tools/column_counts.py [c2|c4]       # on the GPU box

Every k_vote wave adds up, per count-table item, the counted atomic lane-operations 17 columns per entry would be, those of
the table's set columns, and those of the tables with all 17 set (ppf_match_stats.phase_clocks[0..2] of that build)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from yolo_ppf_pose_estimation_amd import workloads as W
    from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
    from yolo_ppf_pose_estimation_amd.device import Workspace
    cfg = sys.argv[1] if len(sys.argv) > 1 else "c2"
    bottle = W.bottle()
    step, scene = (W.C4["model_step"], W.c4_scene()) if cfg == "c4" else (W.C2["model_step"], W.c2_scene())
    det = PPF3DDetector(step, W.REL_DISTANCE).trainModel(bottle)
    d = torch.from_numpy(scene).cuda()
    ws = Workspace(timing=True)
    st = None
    for _ in range(2):
        ws.match_device(det, d.data_ptr(), scene.shape[0], 6, W.SCENE_STEP, W.REL_DISTANCE, presampled=True)
        st = ws.results(scene.shape[0])["stats"]
    dense, cols, full = st["phase_clocks"][:3]
    if not dense:
        raise SystemExit("no counts: is PPF_HIP_LIB a -DPPF_DIAG_COLUMNS build?")
    print(json.dumps({"config": cfg, "lane_ops_17_columns": dense, "lane_ops_set_columns": cols, "lane_ops_of_tables_with_all_17": full,
                      "mean_nonzero_columns": 17.0 * cols / dense, "share_of_counted_work_in_tables_with_all_17": full / dense,
                      "n_tables": st["n_tables"], "n_lds_atomics": st["n_lds_atomics"], "n_votes": st["n_votes"]}))


if __name__ == "__main__":
    main()
