"""Time ppf_volume_mesh_components beside ppf_depth_volume_mesh on the same scanned volumes: tools/volume_mesh_timing.py's stream
(the reference's frame and seven seeded camera motions of it, integrated at their true poses) in the default volume's cube at
128^3 and 256^3 voxels.  The yardstick is ppf_depth_volume_mesh, which the parent commit has: the ratio components / mesh is
reported per round and per size.

Routes alternate in one process after one warm-up (median and p10 - p90 of `--reps`, default 50).  Before anything is timed both
routes are held to the numpy oracles' bytes (tests/volume_mesh_oracle.py at 128^3; tests/mesh_components_oracle.py at both
sizes, on the mesh the device made: output vertices and triangles, labels, the info records and the counts, for the defaults
and for min_triangles = 100).

Beside each time: the bytes the call streams and those bytes at the 6.3 TB/s the microarchitecture guide gives as achievable
(the floor).  components: the triangles (12 bytes) read by the unite, sum, flag and write passes and the vertices (24 bytes) by
the flatten, sum and write passes; the per-vertex scratch (68 bytes of sums, parent, root and flags cleared or written once and
read once, 40 bytes of sort keys and values eight times over); the edge table (12 bytes a slot cleared, then read once; its
probes are taken as cache hits); the output written.  The scans' partial sums are left out.  Every time includes the launches,
the clears, both waits and the allocation of the result.  The launches are also timed alone: the same call on an empty mesh,
whose passes have nothing to stream.  No counter pass or kernel trace is taken.
Writes profiles/r32_mesh_components_timing.json (or --out).  Run it under a time limit of its own:
  timeout -k 10 600 python tools/mesh_components_timing.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import depth_volume_oracle as O  # noqa: E402
import mesh_components_oracle as MC  # noqa: E402
import volume_mesh_oracle as M  # noqa: E402
from depth_motion_timing import summary, timed  # noqa: E402
from depth_volume_timing import ACHIEVABLE, floor_entry, stream, volume_params  # noqa: E402
from yolo_ppf_pose_estimation_amd.cloud_processor import DepthVolume, VolumeMesh  # noqa: E402


def hold_components(mesh, v, t):
    measured = MC.measure(v, t)
    for kw in (dict(), dict(min_triangles=100)):
        want = MC.select(measured, **kw)
        out, info, lab, st = mesh.components(labels=True, max_info=64, return_stats=True, **kw)
        assert all(st[k] == want[k] for k in MC.COUNTS), (st, {k: want[k] for k in MC.COUNTS})
        assert (st["n_launches"], st["n_host_syncs"]) == (MC.N_LAUNCHES, MC.N_HOST_SYNCS)
        assert out.vertices().tobytes() == want["out_vertices"].tobytes() and out.triangles().tobytes() == want["out_triangles"].tobytes()
        assert lab.tobytes() == want["labels"].tobytes()
        for got, rec in zip(info, want["info"]):
            assert all(got[k] == rec[k] for k in ("n_vertices", "n_triangles", "n_edges", "n_boundary_edges", "n_nonmanifold_edges",
                                                  "first_vertex", "kept", "area")), (got, rec)
            assert got["lo"] == tuple(rec["lo"].tolist()) and got["hi"] == tuple(rec["hi"].tolist())
    return MC.select(measured), st


def run_size(n, frames, poses, intr, reps, hold_mesh):
    import torch
    vp = volume_params(n)
    vol = DepthVolume(vp["dims"], vp["voxel"], vp["origin"], vp["trunc"])
    for f, P in zip(frames, poses):
        vol.integrate(torch.from_numpy(f).cuda(), intr, P)
    mesh, mst = vol.mesh(return_stats=True)
    v, t = mesh.vertices(), mesh.triangles()
    if hold_mesh:
        ora = O.Volume(**vp)
        for f, P in zip(frames, poses):
            O.integrate(ora, f, intr, P)
        wv, wt, wst = M.mesh(ora, 1)
        assert v.tobytes() == wv.tobytes() and t.tobytes() == wt.tobytes() and all(mst[k] == wst[k] for k in wst), n
    full, cst = hold_components(mesh, v, t)
    nv, nt = len(v), len(t)
    slots = 64
    while slots < 6 * nt:
        slots *= 2
    i = full["info"]
    res = {"dims": [n, n, n], "n_vertices": nv, "n_triangles": nt, "edge_table_slots": slots,
           "components": {"n_components": full["n_components"], "largest_triangles": [int(x) for x in i["n_triangles"][:3]],
                          "largest_area_m2": [float(x) for x in i["area"][:3]], "n_launches": int(cst["n_launches"]),
                          "n_host_syncs": int(cst["n_host_syncs"])},
           "equal_to_oracle": ("mesh and components" if hold_mesh else "components, on the device's mesh")}
    print(f"{n}^3: {res}", file=sys.stderr, flush=True)
    empty = VolumeMesh.from_arrays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    routes = {"components": lambda: mesh.components(max_info=64), "components_measure_only": lambda: mesh.components(measure_only=True),
              "components_empty_mesh": lambda: empty.components(), "mesh": lambda: vol.mesh()}
    for fn in routes.values():
        fn()
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for key, fn in routes.items():
            o, dt = timed(fn)
            ms[key].append(dt)
            del o
    streamed = {"mesh_read": 4 * nt * 12 + 3 * nv * 24, "scratch": nv * (2 * 68 + 8 * 2 * 40), "edge_table": 2 * slots * 12,
                "output": nv * 24 + nt * 12}
    for key, val in ms.items():
        res[key + "_ms"] = summary(val)
    res["components_bytes"] = dict(streamed, **floor_entry(res["components_ms"], sum(streamed.values())))
    res["components_over_mesh"] = summary(np.asarray(ms["components"]) / np.asarray(ms["mesh"]))
    res["launches_and_waits_share"] = round(res["components_empty_mesh_ms"]["median"] / res["components_ms"]["median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_mesh_components_timing.json"))
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_components_timing.py needs a GPU")
    frames, poses, intr = stream()
    doc = {"tool": "tools/mesh_components_timing.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "achievable_bytes_per_s": ACHIEVABLE, "reps": a.reps,
           "sizes": [run_size(128, frames, poses, intr, a.reps, True), run_size(256, frames, poses, intr, a.reps, False)]}
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
