"""Time ppf_cloud_from_mesh: the box (12 triangles, every draw through the large path), the torus of 96 x 48
quads and a latitude-longitude sphere of at least 300,000 triangles (small path only), each at two spacings that give about
20,000 and about 1,000,000 rows, with visibility on and off.  There is no earlier implementation, so no ratio is taken and no
time is asserted.

Each route is first held to the numpy oracle's bytes (tests/mesh_oracle.py): the rows' SHA-256 and every count (the oracle takes
about a quarter of a minute over the twelve routes); that call is the warm-up.  Then `--reps` (default 50) rounds in which
the routes alternate; the median with p10 - p90.

Beside each time: the bytes the call streams -- the mesh uploaded and read by the per-triangle kernels (once more per view with
visibility), the offsets, the maps cleared and read, the rows written, read by the visibility test and moved by the scatter --
those bytes at the 6.3 TB/s the microarchitecture guide gives as achievable (the floor), and the median over that floor.  The
time of a call includes its upload, its launches and both waits; what takes the time inside a call is only separated by
`--trace`, which runs every route once so that a kernel trace of the process (a run of its own) gives the kernels' shares,
which `--trace-csv` then puts beside the times:
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o mesh -- python tools/mesh_sample_timing.py --trace
Writes the next free profiles/rNN_mesh_sample_timing.json (or --out).  Run it under a time limit of its own:
  timeout -k 10 600 python tools/mesh_sample_timing.py
"""
import argparse
import glob
import hashlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mesh_cases as MC  # noqa: E402
import mesh_oracle as MO  # noqa: E402

ACHIEVABLE = 6.3e12   # bytes per second
COUNTS = ("n_triangles", "n_degenerate", "n_sampled", "n_hidden", "n_flipped", "n_rows", "n_large")
MAX_ROWS = 1 << 21


def meshes():
    return {"box": MC.box(), "torus 96x48": MC.torus(nu=96, nv=48), "sphere 388x388": MC.sphere(388, 388)}


def routes():
    out = []
    for name, (V, T) in meshes().items():
        _, _, _, _, L, live = MO.triangles_geom(V, T)
        area = float(np.sum(0.5 * L[live]))
        for rows in (20_000, 1_000_000):
            spacing = float(np.float32(np.sqrt(area / rows)))
            for vis in (1, 0):
                out.append(dict(key=f"{name} | {rows} rows | visibility {'on' if vis else 'off'}", mesh=name, spacing=spacing, visibility=vis))
    return out


def oracle_digest(V, T, r):
    o = MO.mesh_sample(V, T, r["spacing"], visibility=r["visibility"], orient=r["visibility"], max_rows=MAX_ROWS)
    return dict(sha256=hashlib.sha256(o["rows"].tobytes()).hexdigest(), **{k: int(o["stats"][k]) for k in COUNTS})


def next_profile():
    taken = [int(m.group(1)) for p in glob.glob(os.path.join(ROOT, "profiles", "r*_*")) for m in [re.match(r"r(\d+)_", os.path.basename(p))] if m]
    return os.path.join(ROOT, "profiles", f"r{max(taken, default=0) + 1:02d}_mesh_sample_timing.json")


def streamed_bytes(V, T, st, vis, R=256):
    """what a call moves through HBM, counted once per pass that streams it"""
    nt, rows, kept = len(T), st["n_sampled"], st["n_rows"]
    mesh = V.nbytes + T.nbytes
    b = 2 * mesh + nt * 9 + 2 * (nt + 1) * 4 + rows * 24      # upload, k_mesh_tri, its outputs, the scan, k_mesh_sample's rows
    if vis:
        maps = 26 * R * R * 4
        b += 26 * (nt * 13) + 2 * maps + rows * 24 + rows * 4   # 26 passes over indices and flags, the maps cleared and read, the test
        b += 3 * (rows + 1) * 4 + rows * 24 + kept * 28             # the flags scanned, the scatter
    return int(b)


def trace_shares(path):
    """the kernel trace of a `--trace` run (rocprofv3 --kernel-trace --output-format csv) cut into its routes: a call is 17 launches
    of k_mesh_* and k_scan_* with visibility and 8 without, in the order of routes(); microseconds per kernel and call"""
    import csv
    rows = [r for r in csv.DictReader(open(path)) if re.search(r"k_mesh_|k_scan_", r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out, at = {}, 0
    for r in routes():
        n = 17 if r["visibility"] else 8
        part, at = rows[at:at + n], at + n
        assert len(part) == n, "the trace holds fewer launches than the routes make"
        us = {}
        for k in part:
            name = re.search(r"k_(mesh|scan)_\w+", k["Kernel_Name"]).group(0)
            us[name] = round(us.get(name, 0.0) + (int(k["End_Timestamp"]) - int(k["Start_Timestamp"])) / 1e3, 2)
        out[r["key"]] = {"kernels_us": us, "kernels_total_us": round(sum(us.values()), 2)}
    assert at == len(rows), "the trace holds more launches than the routes make"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--trace", action="store_true", help="run every route once and stop: for a kernel trace of the process")
    ap.add_argument("--trace-csv", default=None, help="the kernel trace of a --trace run: its per-kernel times go into the document")
    a = ap.parse_args()
    M, R = meshes(), routes()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_sample_timing.py needs a GPU")
    from depth_motion_timing import summary, timed
    from yolo_ppf_pose_estimation_amd.cloud_processor import DeviceCloud

    def call(r):
        V, T = M[r["mesh"]]
        return DeviceCloud.from_mesh(V, T, r["spacing"], visibility=bool(r["visibility"]), orient=bool(r["visibility"]), max_rows=MAX_ROWS,
                                     return_stats=True)

    if a.trace:
        for r in R:
            call(r)
        torch.cuda.synchronize()
        return
    doc = {"tool": "tools/mesh_sample_timing.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "achievable_bytes_per_s": ACHIEVABLE, "map_size": 256, "routes": {}}
    for r in R:
        V, T = M[r["mesh"]]
        want = oracle_digest(V, T, r)
        cloud, st = call(r)
        got = dict(sha256=hashlib.sha256(cloud.rows().tobytes()).hexdigest(), **{k: int(st[k]) for k in COUNTS})
        assert got == want, (r["key"], got, want)
        doc["routes"][r["key"]] = {"triangles": len(T), "spacing": r["spacing"], **{k: got[k] for k in COUNTS}, "n_launches": st["n_launches"],
                                   "n_host_syncs": st["n_host_syncs"], "equal_to_oracle": "rows (SHA-256) and counts"}
        print(f"{r['key']}: {doc['routes'][r['key']]}", file=sys.stderr, flush=True)
        del cloud
    ms = {r["key"]: [] for r in R}
    for _ in range(a.reps):
        for r in R:
            o, dt = timed(lambda: call(r))
            ms[r["key"]].append(dt)
            del o
    for r in R:
        e = doc["routes"][r["key"]]
        e["ms"] = summary(ms[r["key"]])
        nbytes = streamed_bytes(*M[r["mesh"]], e, r["visibility"])
        floor = nbytes / ACHIEVABLE * 1e3
        e["streamed_bytes"], e["floor_ms"], e["median_over_floor"] = nbytes, round(floor, 5), round(e["ms"]["median"] / floor, 1)
    doc["not_separated"] = ("a call's time holds the upload of the mesh, 8 or 17 launches, the clear of the maps, two blocking waits and the "
                            "allocation of the cloud; only the kernels are separated, by a kernel trace of `--trace`, a run of its own, "
                            "where one was taken: the rest is the difference and was not split further")
    if a.trace_csv:
        for key, v in trace_shares(a.trace_csv).items():
            doc["routes"][key].update(v)
    print(json.dumps(doc, indent=1))
    if not a.no_write:
        with open(a.out or next_profile(), "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
