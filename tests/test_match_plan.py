"""match_plan, the pure function that cuts a match call into batches of reference points and sizes its hit pools and LDS
areas, through ppf_debug_match_plan (host only, no GPU).  Every output field is compared for exact equality with a
restatement of the sizing arithmetic in Python, written from the formulas and sharing no code with the library: IEEE doubles
and integers in a fixed order on both sides, int() for the truncating casts.  Also the two structs' layout as a C++ compiler
sees include/ppf_hip.h against their ctypes mirrors.

The restatement keeps the clamp `batch <= 2.0e9 / hits_per_ref` that the library replaced by a static_assert
(HIT_BYTES_BUDGET / HIT_SCRATCH_BYTES < 2.0e9): every case below would differ if it could bind.

"More paired points than one call can group" starts where (pair_chunks + 2 rounded down to even) * 8 bytes no longer fit
beside the bucket counters of a round: with a full round of 36,000 buckets at pair_chunks = 2,224, i.e. 6,829,057 paired
points; 2.7 million (886 chunks) still fit."""
import ctypes as C
import os
import subprocess

import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import MatchPlanIn, MatchPlanOut, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# csrc/ppf_match_kernels.h, ppf_device_mem.h, ppf_core.h (default build)
WG_HITS = 256 * 12                      # PAIR_BLOCK * PAIRS_PER_THREAD
GROUP_MAX_BUCKETS = 36000
HIT_BYTES_BUDGET = 4 << 30
HIT_SCRATCH_BYTES = 8.0 + 8.0 + 2.0 + 16.0 / 6.0
AGG_SCRATCH = ((64 + 1) * 20 + 15) // 16 * 16
TBL_BYTES = AGG_SCRATCH + 1024 + 192
TBL_FRAC_MAX = 1.0 / 24 + 1.0 / 191
TBL_FRAC_START = 0.02
LDS_BYTES = 160 * 1024
RUN_SEG, RUN_SEG_MAX = 704, 1024
U32 = 0xFFFFFFFF


def vote_lds_fixed(run_seg):
    return 256 + ((run_seg + 1) * 24 + 15) // 16 * 16 + 16 * AGG_SCRATCH


def want_plan(n_ref, n_paired, hit=0.25, run=0.4, tbl=TBL_FRAC_START, count_tables=1, batch_refs_cap=0, round_buckets_cap=0,
              run_seg_cap=0, n_buckets=20000, tile_refs=2000, num_angles=30):
    """the parent's sizing lines, restated; a dict of the outputs, or the words the error message must hold"""
    o = {}
    o["pair_chunks"] = pc = (n_paired + WG_HITS - 1) // WG_HITS
    round_cap = min(round_buckets_cap, GROUP_MAX_BUCKETS) if round_buckets_cap > 0 else GROUP_MAX_BUCKETS
    o["n_rounds"] = max(1, (n_buckets + round_cap - 1) // round_cap)
    o["round_buckets"] = min(max(n_buckets, 1), round_cap)
    frac = min(1.0, max(hit, 1e-3))
    hits_per_ref = max(64.0, frac * float(n_paired))
    tbl_frac = 0.0 if not count_tables else TBL_FRAC_MAX if frac >= 1.0 else min(TBL_FRAC_MAX, tbl)
    batch = int(min(float(n_ref), max(1.0, float(HIT_BYTES_BUDGET) / (hits_per_ref * (HIT_SCRATCH_BYTES + tbl_frac * TBL_BYTES)))))
    batch = int(min(float(batch), max(1.0, 2.0e9 / hits_per_ref)))
    batch = min(batch, 32768)
    if batch_refs_cap > 0:
        batch = min(batch, batch_refs_cap)
    worst_case = frac >= 1.0
    est = hits_per_ref * float(batch)
    stripe_bits = 6
    while stripe_bits > 0 and ((batch * pc) >> stripe_bits) < 512:
        stripe_bits -= 1
    if worst_case:
        stripe_bits = 0
    n_stripes = 1 << stripe_bits
    if worst_case:
        stripe_cap = int(min(4.0e9 / n_stripes, float(batch) * pc * WG_HITS))
    else:
        stripe_cap = (int(est / n_stripes * 1.04) + 2 * WG_HITS) & U32
    sorted_cap = int(min(4.0e9, est + 4096.0))
    run_cap = sorted_cap if worst_case else int(min(float(sorted_cap), max(est * min(1.0, run), 64.0 * batch) + 1024.0))
    table_cap = 1 if not count_tables else int(min(1.0e9, max(est * (TBL_FRAC_MAX if worst_case else tbl_frac), 4.0 * batch) + 256.0))
    o.update(batch=batch, n_batches=(n_ref + batch - 1) // batch, stripe_bits=stripe_bits, stripe_cap=stripe_cap, sorted_cap=sorted_cap,
             run_cap=run_cap, table_cap=table_cap)
    acc_words = 64 + 2 * ((num_angles + 1) | 1) + ((tile_refs + 1) // 2) * num_angles + 1
    least = vote_lds_fixed(RUN_SEG) + acc_words * 4
    run_seg = RUN_SEG if least >= LDS_BYTES else min(RUN_SEG_MAX, RUN_SEG + 64 * ((LDS_BYTES - least) // (64 * 24)))
    if run_seg_cap > 0:
        run_seg = max(64, min(run_seg, run_seg_cap // 64 * 64))
    o["run_seg"] = run_seg
    o["vote_lds"] = vote_lds_fixed(run_seg) + acc_words * 4
    if o["vote_lds"] > LDS_BYTES:
        return f"match: model tile of {tile_refs} reference points does not fit the LDS accumulator"
    o["group_lds"] = ((o["round_buckets"] + 1) & ~1) * 4 + ((pc + 2) & ~1) * 4 * 2
    if o["group_lds"] + 2048 > LDS_BYTES:
        return f"match: {n_paired} paired points are more than one call can group"
    return o


def got_plan(n_ref, n_paired, hit=0.25, run=0.4, tbl=TBL_FRAC_START, count_tables=1, batch_refs_cap=0, round_buckets_cap=0,
             run_seg_cap=0, n_buckets=20000, tile_refs=2000, num_angles=30):
    pin = MatchPlanIn(n_ref, n_paired, hit, run, tbl, count_tables, batch_refs_cap, round_buckets_cap, run_seg_cap, n_buckets, tile_refs,
                      num_angles)
    out = MatchPlanOut()
    out.batch = 77   # garbage a failing call must clear
    s = lib().ppf_debug_match_plan(C.byref(pin), C.byref(out))
    fields = {f: getattr(out, f) for f, _ in MatchPlanOut._fields_}
    if s != _capi.PPF_OK:
        assert s == _capi.PPF_ERR_INVALID and not any(fields.values())
        return _capi.last_error()
    return fields


C2 = dict(n_ref=2500, n_paired=50000)
CASES = {
    "one_point": dict(n_ref=1, n_paired=1),
    "c2": C2,
    "c2_s2b_edge_cloud": dict(n_ref=2500, n_paired=7001),
    "worst_case": dict(n_ref=2500, n_paired=200000, hit=1.0),
    "worst_case_tables_off": dict(n_ref=2500, n_paired=200000, hit=1.0, count_tables=0),
    "hit_above_one": dict(n_ref=300, n_paired=9000, hit=1.5),
    "grid_y_cap": dict(n_ref=100000, n_paired=200),
    "batch_refs_cap": dict(n_ref=503, n_paired=20000, batch_refs_cap=37),
    "tables_off": dict(count_tables=0, **C2),
    "tbl_frac_above_max": dict(tbl=0.3, **C2),
    "hit_floor": dict(hit=1e-6, **C2),
    "hit_0002": dict(hit=0.002, **C2),
    "run_frac_above_one": dict(run=1.7, **C2),
    "run_floor": dict(run=1e-5, n_ref=40000, n_paired=3000, hit=0.01),
    "three_rounds": dict(n_buckets=100000, **C2),
    "capped_rounds": dict(n_buckets=100000, round_buckets_cap=500, **C2),
    "round_cap_above_max": dict(n_buckets=100000, round_buckets_cap=50000, **C2),
    "no_buckets": dict(n_buckets=0, **C2),
    "staging_64": dict(run_seg_cap=64, **C2),
    "staging_100": dict(run_seg_cap=100, **C2),
    "staging_1": dict(run_seg_cap=1, **C2),
    "small_tile_full_staging": dict(tile_refs=400, **C2),
    "many_stripes": dict(n_ref=40000, n_paired=500000, hit=0.004),
    "one_ref_per_batch": dict(n_ref=5, n_paired=60_000_000, hit=0.9, n_buckets=100),
    "largest_groupable_full_round": dict(n_ref=7, n_paired=2223 * WG_HITS, hit=1.0, n_buckets=36000),
    "2p7_million_still_fits": dict(n_ref=7, n_paired=886 * WG_HITS, n_buckets=36000),
    "too_many_paired_points": dict(n_ref=7, n_paired=2223 * WG_HITS + 1, n_buckets=36000),
    "largest_tile": dict(tile_refs=2084, **C2),
    "tile_leaves_no_staging": dict(tile_refs=2085, **C2),
    "tile_fits_only_with_less_staging": dict(tile_refs=2085, run_seg_cap=64, **C2),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_equals_the_restated_arithmetic(name):
    assert got_plan(**CASES[name]) == want_plan(**CASES[name])


def test_corners_are_what_the_formulas_say():
    """the figures worked out by hand, so that the restatement is itself pinned"""
    p = got_plan(n_ref=1, n_paired=1)
    assert (p["batch"], p["n_batches"], p["stripe_bits"], p["pair_chunks"]) == (1, 1, 0, 1)
    assert p["sorted_cap"] == 64 + 4096 and p["stripe_cap"] == int(64 * 1.04) + 2 * WG_HITS   # the 64-hit floor
    assert got_plan(**C2)["n_batches"] == 1
    p = got_plan(n_ref=2500, n_paired=200000, hit=1.0)
    assert p["stripe_bits"] == 0 and p["stripe_cap"] == p["batch"] * p["pair_chunks"] * 3072
    assert p["run_cap"] == p["sorted_cap"] == 200000 * p["batch"] + 4096
    assert p["table_cap"] == int(200000.0 * p["batch"] * TBL_FRAC_MAX + 256.0)
    p = got_plan(n_ref=100000, n_paired=200)
    assert (p["batch"], p["n_batches"]) == (32768, 4)
    p = got_plan(n_ref=503, n_paired=20000, batch_refs_cap=37)
    assert (p["batch"], p["n_batches"]) == (37, 14)
    assert got_plan(count_tables=0, **C2)["table_cap"] == 1
    assert got_plan(n_buckets=100000, **C2)["n_rounds"] == 3
    p = got_plan(n_buckets=100000, round_buckets_cap=500, **C2)
    assert (p["n_rounds"], p["round_buckets"]) == (200, 500)
    assert got_plan(**CASES["too_many_paired_points"]) == "match: 6829057 paired points are more than one call can group"
    assert got_plan(**CASES["tile_leaves_no_staging"]) == "match: model tile of 2085 reference points does not fit the LDS accumulator"
    assert isinstance(got_plan(**CASES["tile_fits_only_with_less_staging"]), dict)


def test_bad_arguments():
    ok = MatchPlanIn(10, 10, 0.25, 0.4, 0.02, 1, 0, 0, 0, 100, 100, 30)
    out = MatchPlanOut()
    f = lib().ppf_debug_match_plan
    assert f(C.byref(ok), C.byref(out)) == _capi.PPF_OK
    assert f(None, C.byref(out)) == _capi.PPF_ERR_INVALID and f(C.byref(ok), None) == _capi.PPF_ERR_INVALID
    for field, v in (("n_ref", 0), ("n_paired", 0), ("n_paired", -5), ("tile_refs", 0), ("num_angles", 0), ("batch_refs_cap", -1),
                     ("round_buckets_cap", -1), ("run_seg_cap", -1)):
        bad = MatchPlanIn.from_buffer_copy(ok)
        setattr(bad, field, v)
        assert f(C.byref(bad), C.byref(out)) == _capi.PPF_ERR_INVALID, field
        assert "ppf_debug_match_plan" in _capi.last_error() and out.batch == 0


def test_plan_struct_layouts_match_the_header(tmp_path):
    structs = [("ppf_debug_match_plan_in", MatchPlanIn), ("ppf_debug_match_plan_out", MatchPlanOut)]
    expr, got = [], []
    for cname, cls in structs:
        expr.append(f"sizeof({cname})")
        got.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            expr.append(f"offsetof({cname}, {f})")
            got.append(getattr(cls, f).offset)
    expr.append("PPF_ABI_VERSION")
    got.append(4)
    src = tmp_path / "plan_sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ppf_hip.h"\nint main(){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "plan_sz"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
