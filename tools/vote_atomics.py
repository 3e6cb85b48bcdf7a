#!/usr/bin/env python3
"""n_votes and n_lds_atomics of the C2 step with direct votes and with count tables, on the library PPF_HIP_LIB names
(default: the in-tree build).  With direct votes the atomics count is a function of the work items alone: two builds that
form the same items print the same number.  With count tables it varies from call to call on one build (which hits of a long
run share a table decides the tables' column masks).

    PPF_HIP_LIB=build_var/other.so python tools/vote_atomics.py       # on the GPU box"""
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
    det = PPF3DDetector(W.C2["model_step"], W.REL_DISTANCE).trainModel(W.bottle())
    scene = W.c2_scene()
    d = torch.from_numpy(scene).cuda()
    out = {}
    for mode in (1, 0):
        ws = Workspace()
        st = None
        for _ in range(2):  # the second call: pools sized, no repeat
            ws.match_device(det, d.data_ptr(), scene.shape[0], 6, W.SCENE_STEP, W.REL_DISTANCE, presampled=True, vote_mode=mode)
            st = ws.results(scene.shape[0])["stats"]
        out["direct" if mode else "tables"] = {k: int(st[k]) for k in ("n_votes", "n_lds_atomics", "n_tables", "n_acc32_items")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
