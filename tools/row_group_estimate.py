#!/usr/bin/env python3
"""How many entries of the C2 table cast their counted adds at the same words: the (bucket, row, X) groups behind k_vote's
group records, and what merging them is worth at a cap of K entries per record (numpy, CPU only; statistics, not parity: the
crop's pair keys are binned with numpy's arccos as in tools/vote_cost_model.py, and X is formed in fp32 without the table
build's fp64 second look at cell edges).

Entries that share bucket, model row and X (the count-table shift floor(alpha_m * A / (4 pi) + A / 2) carried in the row code)
differ only in the table row T[q] they take their counts from.  A record of up to K of them casts one set of (v_perm_b32,
ds_add_u32) pairs instead of one per entry: a group of g entries keeps ceil(g / K) of its g sets.

Printed: the group-size histogram of the model, the share of pairs kept per cap, unweighted (every entry once) and weighted by
what the kernel does on a sample of the crop's reference points -- count tables x entries of every (reference point, bucket)
run that votes through count tables (>= 24 hits, >= 32 pair records) -- and the statistics of the buckets those runs visit.

    python tools/row_group_estimate.py [--refs 12] [--json out.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_lib as O  # noqa: E402
from vote_cost_model import murmur_low32  # noqa: E402
from yolo_ppf_pose_estimation_amd import workloads as W  # noqa: E402

CAPS = (2, 3, 4, 6, 8)
AGG_MIN_HITS, AGG_MIN_RECORDS, AGG_SUB = 24, 32, 191


def records_for(entries):
    return 32 * (entries // 64) + np.minimum(32, entries % 64)


def hits_per_slot(scene, r, astep, dstep, slots):
    """Hits of reference point r per hash slot (tools/vote_cost_model.runs_of_reference, without the bucket sizes)."""
    P = scene[:, :3].astype(np.float64); Nn = scene[:, 3:].astype(np.float64)
    d = P - P[r]; f3 = np.linalg.norm(d, axis=1); ok = f3 > 0
    dn = d[ok] / f3[ok, None]
    f0 = np.arccos(np.clip(dn @ Nn[r], -1, 1)); f1 = np.arccos(np.clip((Nn[ok] * dn).sum(1), -1, 1))
    f2 = np.arccos(np.clip(Nn[ok] @ Nn[r], -1, 1))
    k = murmur_low32((f0 / astep).astype(np.int64), (f1 / astep).astype(np.int64), (f2 / astep).astype(np.int64),
                     (f3[ok] / dstep).astype(np.int64)) % slots
    return np.unique(k, return_counts=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=12)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ora = O.OracleDetector(W.C2["model_step"], W.REL_DISTANCE).train_model(W.bottle())
    info = ora.info(); N, slots, A = info["n_ref"], info["slots"], info["num_angles"]
    hsh, alp = ora.pairs()
    off = ~np.eye(N, dtype=bool)
    rows = np.nonzero(off)[0]
    slot = (hsh[off].astype(np.uint64) % np.uint64(slots)).astype(np.int64)
    X = np.floor(alp[off].astype(np.float32) * np.float32(A / (4 * math.pi)) + np.float32(0.5 * A)).astype(np.int64)
    # one group per (bucket, row, X); one tile on C2, so a bucket is a (tile, bucket)
    key = (slot * N + rows) * 64 + X
    gkey, gsize = np.unique(key, return_counts=True)
    gslot = gkey // (64 * N)
    bucket_entries = np.bincount(slot, minlength=slots)
    bucket_groups = np.bincount(gslot, minlength=slots)
    kept = {K: np.bincount(gslot, weights=(gsize + K - 1) // K, minlength=slots) for K in CAPS}  # records per bucket at cap K
    rows_per_bucket = np.bincount(np.unique(slot * N + rows) // N, minlength=slots)
    x_per_row = bucket_groups / np.maximum(rows_per_bucket, 1)

    scene = W.c2_scene()
    n_ref_total = scene.shape[0] // 20
    refs = [int(k * n_ref_total / a.refs) * 20 for k in range(a.refs)]
    weight = np.zeros(slots)   # count tables that visit the bucket, over the sampled reference points
    for r in refs:
        s, m = hits_per_slot(scene, r, info["angle_step"], info["distance_step"], slots)
        agg = (m >= AGG_MIN_HITS) & (records_for(bucket_entries[s]) >= AGG_MIN_RECORDS)
        np.add.at(weight, s[agg], (m[agg] + AGG_SUB - 1) // AGG_SUB)
    visited = weight > 0
    out = {
        "model": {"n_ref": int(N), "entries": int(bucket_entries.sum()), "groups": int(len(gsize)),
                  "mean_group_size": float(gsize.mean()),
                  "group_size_histogram": {str(g): int(c) for g, c in enumerate(np.bincount(np.minimum(gsize, 17))) if g and c},
                  "group_size_histogram_note": "17 = 17 entries and more"},
        "refs_sampled": len(refs),
        "visited_buckets": {
            "count": int(visited.sum()),
            "entries_mean_median_p90_max": [float(np.average(bucket_entries[visited], weights=weight[visited])),
                                            float(np.median(bucket_entries[visited])),
                                            float(np.percentile(bucket_entries[visited], 90)), int(bucket_entries[visited].max())],
            "entries_per_row_weighted": float((weight * bucket_entries).sum() / max((weight * rows_per_bucket).sum(), 1)),
            "distinct_x_per_row_weighted": float(np.average(x_per_row[visited], weights=(weight * rows_per_bucket)[visited])),
            "weighted_mean_group_size": float((weight * bucket_entries).sum() / max((weight * bucket_groups).sum(), 1)),
        },
        "pairs_kept_per_cap": {str(K): {"unweighted": float(kept[K].sum() / bucket_entries.sum()),
                                        "weighted_by_tables_x_entries": float((weight * kept[K]).sum() / max((weight * bucket_entries).sum(), 1))}
                               for K in CAPS},
        "group_record_bytes_at_cap_4": int(8 * kept[4][records_for(bucket_entries) >= AGG_MIN_RECORDS].sum()),
    }
    print(json.dumps(out, indent=1))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
