"""Regenerate tests/golden/select_two_bottles.npz: the ORACLES' refined poses for three detections of the synthetic frame of
tests/test_gpu_frame.py::_render_frame (two bottles and a box in front of a plane): the box of bottle 0, the box of bottle 1
and the union of the two, each matched against the bottle model.

    prep oracles (crop -> voxel 4 mm -> outlier removal (50, 1.0) -> normals (30) -> edges (0.03))
    -> OracleDetector(0.05, 0.05).train_model(bottle) -> match_S2B(scene, edge, 0.05, 0.05) -> top 8
    -> icp_refine with the default ICP parameters

    python tests/golden/make_select_fixture.py        (CPU only; about 30 s)

The file holds poses [3, 8, 4, 4], n_poses [3], boxes [3, 4] and the two bottles' true poses: what ppf_select_frame has to
turn into exactly one pose per bottle."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_lib as O  # noqa: E402
from test_gpu_frame import _render_frame  # noqa: E402

LEAF, TOP, TRAIN = 0.004, 8, (0.05, 0.05)


def union(a, b):
    x0, y0 = min(a[0], b[0]), min(a[1], b[1])
    x1, y1 = max(a[0] + a[2], b[0] + b[2]), max(a[1] + a[3], b[1] + b[3])
    return (x0, y0, x1 - x0, y1 - y0)


def chain():
    bottle = np.load(os.path.join(HERE, "bottle_model_xyzn.npy"))
    scene, depth, boxes, K, objs, _ = _render_frame(bottle)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    boxes = [boxes[0], boxes[1], union(boxes[0], boxes[1])]
    ora = O.OracleDetector(*TRAIN).train_model(bottle)
    poses, n_poses = np.zeros((3, TOP, 4, 4)), np.zeros(3, dtype=np.int32)
    for i, box in enumerate(boxes):
        keep, _ = O.prep_crop(scene, box, depth, intr)
        v = O.prep_voxel(scene[keep], LEAF)
        k2, _, _ = O.prep_sor(v, 50, 1.0)
        v = v[k2]
        n, c = O.prep_normals(v, 30)
        obj = O.prep_to_mat(v, n)
        edge = O.prep_to_mat(v[c > 0.03], n[c > 0.03])
        m = ora.match(obj, edge=edge, relative_scene_sample_step=0.05, relative_scene_distance=0.05, cluster=True)
        top = m["poses"][:TOP]
        P, _, _ = O.icp_refine(bottle, obj, [p["pose"] for p in top])
        n_poses[i] = len(top)
        poses[i, :len(top)] = P
    return dict(poses=poses, n_poses=n_poses, boxes=np.asarray(boxes, dtype=np.int32),
                true_poses=np.array([objs[0][1], objs[1][1]], dtype=np.float64))


if __name__ == "__main__":
    t0 = time.time()
    g = chain()
    np.savez(os.path.join(HERE, "select_two_bottles.npz"), **g)
    print("boxes", g["boxes"].tolist(), "n_poses", g["n_poses"].tolist())
    print("seconds", time.time() - t0)
