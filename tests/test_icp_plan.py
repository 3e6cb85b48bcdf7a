"""icp_plan, the pure function that lays the jobs of one ICP launch sequence out in the shared scratch arrays, schedules
their levels and sizes every launch and the pinned block, through ppf_debug_icp_plan (host only, no GPU).  Every output
field is compared for exact equality with a restatement of the sizing arithmetic in Python, written from the formulas of
icp_register_group and icp_level_desc as they stood before the plan was lifted out of them, and sharing no code with the
library: integers and IEEE doubles in the same order on both sides.  Python's round() rounds ties to even, as lrint does in
the default rounding mode: that is on purpose, and the ties below (5 / 2, 7 / 2) would give other steps and iteration
limits with any other rule.  Also the two structs' layout as a C++ compiler sees include/ppf_hip.h against their ctypes
mirrors.

The pinned block is new with the plan (one allocation where there were four), so its restatement is its specification:
the tick counter in 64 bytes of its own, then the done flags, the states and the table staging, each 16-byte aligned, for
max(jobs, 8) jobs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import IcpPlanIn, IcpPlanOut, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# csrc/ppf_icp_kernels.h, ppf_icp_host.h (default build)
CHUNK, ENTRIES = 64, 28
ROWS_BLOCK = 8192
LEAVES = 4096
MAX_JOBS = 8
NN_ROWS, NN_WAVES = 8, 65536
TAIL_VAL_BYTES = 16 * CHUNK * 9 * 8
SIZEOF_JOB_DESC = 2 * 8 + 8 * 4 + 8 * 8 + 16 * 8    # IcpJobDesc: 240
SIZEOF_LEVEL_DESC = 8 * 4                          # IcpLevelDesc
SIZEOF_STATE = (16 + 16 + 3 + 1 + 4) * 8 + 5 * 4 + 7 * 4 + 6 * 4   # IcpState2: 392


def level_desc(n, nd_all, level):
    """icp_level_desc: [step, ns, nd, step_shift, staged]"""
    div = 2.0 ** level
    num_samples = int(round(n / div))
    step = max(1, int(round(n / float(max(num_samples, 1)))))
    ns, nd = (n + step - 1) // step, (nd_all + step - 1) // step
    shift = -1
    if step & (step - 1) == 0:
        shift = 0
        while (1 << shift) < step:
            shift += 1
    return [step, ns, nd, shift, 1 if ns <= 32768 else 0]


def up16(b):
    return (b + 15) // 16 * 16


def want_plan(jobs, uniform=0, iterations=100, tolerance=0.005, rejection_scale=2.5, num_levels=8):
    """the sizing lines of icp_register_group, restated; jobs is a list of (n, nd_all)"""
    J = len(jobs)
    o = {}
    o["levels_off"] = J * SIZEOF_JOB_DESC
    o["table_bytes"] = o["levels_off"] + J * max(num_levels, 1) * SIZEOF_LEVEL_DESC
    t_src = t_dst = t_sel = t_parts = t_sums = t_sumd = 0
    max_chunks = max_rows_blocks = max_dst_blocks = 0
    offs = []
    for n, nd in jobs:
        chunks_src, chunks_dst = (n + CHUNK - 1) // CHUNK, (nd + CHUNK - 1) // CHUNK
        m = min(n, nd)
        offs.append([t_src * 6, t_dst * 6, t_src, t_dst, t_sel, t_parts, t_sums, t_sumd])
        t_src += n
        t_dst += nd
        t_sel += m
        t_parts += (m + CHUNK - 1) // CHUNK * ENTRIES
        t_sums += chunks_src * 3
        t_sumd += chunks_dst * 3
        max_chunks = max(max_chunks, chunks_src + chunks_dst)
        nb_dst, nb_src = (nd + ROWS_BLOCK - 1) // ROWS_BLOCK, (n + ROWS_BLOCK - 1) // ROWS_BLOCK
        max_rows_blocks = max(max_rows_blocks, nb_dst + nb_src)
        max_dst_blocks = max(max_dst_blocks, nb_dst)
    o.update(t_src=t_src, t_dst=t_dst, t_sel=t_sel, t_parts=t_parts, t_sums=t_sums, t_sumd=t_sumd, first_off=offs[0], last_off=offs[-1],
             max_chunks=max_chunks, max_rows_blocks=max_rows_blocks, max_dst_blocks=max_dst_blocks)
    o.update(g_start=J * (LEAVES + 64), g_cur=J * LEAVES, g_box2=J * LEAVES * 2, g_box1u=J * 64 * 8, state=max(J, MAX_JOBS),
             bb_parts=t_sumd * 2)
    o["h_done_off"] = 64
    o["h_state_off"] = o["h_done_off"] + up16(o["state"] * 4)
    o["h_tables_off"] = o["h_state_off"] + up16(o["state"] * SIZEOF_STATE)
    o["pinned_bytes"] = o["h_tables_off"] + o["table_bytes"]
    o["robust"] = 1 if rejection_scale > 0 else 0
    o["n_levels"] = num_levels
    o["pad0"] = 0
    per_level = ("tol_p", "sum_ns", "tail_lds", "max_iter", "max_ns", "nn_rows", "nn_blocks", "begin_blocks", "uni_p_sel", "uni_p_parts")
    for f in per_level:
        o[f] = [0] * 8
    o["first_level"], o["last_level"] = [[0] * 5 for _ in range(8)], [[0] * 5 for _ in range(8)]
    o["uni"] = [[0] * 7 for _ in range(8)]
    tol = float(np.float32(tolerance))
    for level in range(num_levels):
        o["tol_p"][level] = tol * float(level + 1) * (level + 1)
        o["max_iter"][level] = int(round(iterations / (level + 1)))
        L = [level_desc(n, nd, level) for n, nd in jobs]
        max_ns = max(d[1] for d in L)
        sum_ns = sum(d[1] for d in L)
        o["max_ns"][level], o["sum_ns"][level] = max_ns, sum_ns
        o["tail_lds"][level] = max([TAIL_VAL_BYTES] + [d[1] * 4 if d[4] else 0 for d in L])
        o["begin_blocks"][level] = (max_ns + 255) // 256
        nn_rows = min(NN_ROWS, max(1, sum_ns // NN_WAVES))
        o["nn_rows"][level] = nn_rows
        o["nn_blocks"][level] = (max_ns + 4 * nn_rows - 1) // (4 * nn_rows)
        o["first_level"][level], o["last_level"][level] = L[0], L[-1]
        if uniform:
            n, nd = jobs[0]
            step, ns, nd_l, shift, staged = L[0]
            o["uni"][level] = [ns, nd_l, step, shift, staged, n, nd]   # IcpUniform's order
            o["uni_p_sel"][level] = min(n, nd)
            o["uni_p_parts"][level] = (min(n, nd) + CHUNK - 1) // CHUNK * ENTRIES
    return o


def plain(v):
    return [plain(x) for x in v] if isinstance(v, C.Array) else v


def call_plan(jobs, uniform=0, iterations=100, tolerance=0.005, rejection_scale=2.5, num_levels=8):
    pin = IcpPlanIn()
    for j, (n, nd) in enumerate(jobs[:8]):
        pin.n[j], pin.nd_all[j] = n, nd
    pin.jobs, pin.uniform, pin.iterations, pin.tolerance, pin.rejection_scale, pin.num_levels = (
        len(jobs), uniform, iterations, tolerance, rejection_scale, num_levels)
    out = IcpPlanOut()
    out.t_src = 77   # garbage a failing call must clear
    return lib().ppf_debug_icp_plan(C.byref(pin), C.byref(out)), out


def got_plan(*a, **k):
    s, out = call_plan(*a, **k)
    assert s == _capi.PPF_OK, _capi.last_error()
    return {f: plain(getattr(out, f)) for f, _ in IcpPlanOut._fields_}


OTHER = (7, 9)   # a second, ragged job: its offsets (last_off) are the first job's extents in every array
C1 = (19753, 10395)
CASES = {}
# chunks of 64: sums and partials per started chunk of n, nd_all and min(n, nd_all)
for n, nd in ((1, 1), (64, 64), (65, 65), (1, 65), (65, 1), (64, 65), (65, 64), (64, 1000), (65, 1000), (1000, 64), (1000, 65)):
    CASES[f"chunks_{n}_{nd}"] = dict(jobs=[(n, nd), OTHER])
# row blocks of 8,192
for n, nd in ((8192, 8192), (8193, 8193), (8192, 8193), (8193, 8192)):
    CASES[f"row_blocks_{n}_{nd}"] = dict(jobs=[(n, nd), OTHER])
CASES.update({
    # steps
    "step_tie_5": dict(jobs=[(5, 40)], uniform=1, num_levels=2),
    "steps_of_7": dict(jobs=[(7, 100)], uniform=1, num_levels=4),
    "one_row_8_levels": dict(jobs=[(1, 1)], uniform=1),
    "c1": dict(jobs=[C1] * 5, uniform=1),
    # staging of the level's distances in LDS
    "staged_32768": dict(jobs=[(32768, 500)], num_levels=2),
    "not_staged_32769": dict(jobs=[(32769, 500)], num_levels=2),
    "staged_beside_not_staged": dict(jobs=[(32769, 500), (32768, 600)], num_levels=2),
    "tail_floor_binds": dict(jobs=[(300, 200)]),
    # rows per wave of the neighbour search
    "nn_rows_131071": dict(jobs=[(65536, 100), (65535, 100)], num_levels=1),
    "nn_rows_131072": dict(jobs=[(65536, 100), (65536, 100)], num_levels=1),
    "nn_rows_capped": dict(jobs=[(200000, 3000)] * 8, uniform=1, num_levels=3),
    "nn_rows_reaches_8": dict(jobs=[(65536, 100)] * 8, num_levels=2),
    # iteration limits and tolerances
    "iterations_5": dict(jobs=[C1], iterations=5),
    "iterations_0": dict(jobs=[C1], iterations=0),
    "iterations_7": dict(jobs=[C1], iterations=7, tolerance=0.05),
    "no_levels": dict(jobs=[C1, OTHER], num_levels=0),
    "one_level": dict(jobs=[C1, OTHER], num_levels=1),
    "no_rejection": dict(jobs=[C1], rejection_scale=0.0),
    # jobs
    "one_job": dict(jobs=[(4000, 5030)]),
    "one_job_uniform": dict(jobs=[(4000, 5030)], uniform=1),
    "two_uniform": dict(jobs=[(4001, 5030)] * 2, uniform=1),
    "two_equal_not_uniform": dict(jobs=[(4001, 5030)] * 2),
    "two_ragged": dict(jobs=[(4001, 977), (130, 50000)]),
    "eight_ragged": dict(jobs=[(4001, 977), (130, 50000), (1, 1), (64, 65), (8193, 8192), (19753, 10395), (5, 7), (777, 40000)]),
    "eight_uniform": dict(jobs=[(1237, 997)] * 8, uniform=1),
})


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_equals_the_restated_arithmetic(name):
    assert got_plan(**CASES[name]) == want_plan(**CASES[name])


@pytest.mark.parametrize("name", ["one_job_uniform", "two_uniform", "eight_uniform", "c1", "nn_rows_capped"])
def test_uniform_pitches_give_the_tables_offsets(name):
    """icp_pass_geom<false> places job j at j times a pitch taken from IcpUniform; icp_pass_geom<true> reads the job's
    table entry.  Both must name the same place, for every offset the per-pass kernels use."""
    p = got_plan(**CASES[name])
    j = len(CASES[name]["jobs"]) - 1
    o_src0, o_dst0, o_best, o_owner, o_sel, o_parts = p["last_off"][:6]
    assert p["n_levels"] >= 1
    for level in range(p["n_levels"]):
        ns, nd, step, shift, staged, n, nd_all = p["uni"][level]
        assert (j * n * 6, j * nd_all * 6, j * n, j * nd_all) == (o_src0, o_dst0, o_best, o_owner)
        assert (j * p["uni_p_sel"][level], j * p["uni_p_parts"][level]) == (o_sel, o_parts)
        assert [step, ns, nd, shift, staged] == p["first_level"][level] == p["last_level"][level]
    assert p["first_off"] == [0] * 8


def test_corners_are_what_the_formulas_say():
    """the figures worked out by hand, so that the restatement is itself pinned"""
    p = got_plan([(5, 40)], num_levels=2)
    assert p["first_level"][1] == [2, 3, 20, 1, 1]                      # 5 / 2 = 2.5 samples -> 2, 5 / 2 = 2.5 -> step 2
    p = got_plan([(7, 100)], num_levels=4)
    assert [d[0] for d in p["first_level"][:4]] == [1, 2, 4, 7]        # 7/2 = 3.5 -> 4 samples, 7/4 -> 2; 1.75 -> 2, 3.5 -> 4; 0.875 -> 1, 7
    assert [d[3] for d in p["first_level"][:4]] == [0, 1, 2, -1]
    assert [d[1] for d in p["first_level"][:4]] == [7, 4, 2, 1] and [d[2] for d in p["first_level"][:4]] == [100, 50, 25, 15]
    p = got_plan([(1, 1)])
    assert p["first_level"] == [[1, 1, 1, 0, 1]] * 8                    # num_samples rounds to 0 from level 1 on
    assert p["tail_lds"] == [TAIL_VAL_BYTES] * 8 == [73728] * 8 and p["nn_rows"] == [1] * 8 and p["nn_blocks"] == [1] * 8
    assert (p["max_chunks"], p["max_rows_blocks"], p["max_dst_blocks"]) == (2, 2, 1)
    assert (p["t_parts"], p["t_sums"], p["t_sumd"], p["bb_parts"]) == (28, 3, 3, 6)
    assert got_plan([(32768, 500)], num_levels=1)["tail_lds"][0] == 131072
    assert got_plan([(32769, 500)], num_levels=1)["tail_lds"][0] == 73728
    assert got_plan([(65536, 100), (65535, 100)], num_levels=1)["nn_rows"][0] == 1
    p = got_plan([(65536, 100), (65536, 100)], num_levels=1)
    assert (p["nn_rows"][0], p["nn_blocks"][0], p["begin_blocks"][0]) == (2, 8192, 256)
    assert got_plan([(200000, 3000)] * 8, uniform=1, num_levels=1)["nn_rows"][0] == 8
    assert got_plan([C1])["max_iter"] == [100, 50, 33, 25, 20, 17, 14, 12]     # 12.5 -> 12
    assert got_plan([C1], iterations=5)["max_iter"] == [5, 2, 2, 1, 1, 1, 1, 1]  # 2.5 -> 2, 0.625 -> 1
    assert got_plan([C1], iterations=0)["max_iter"] == [0] * 8
    p = got_plan([C1, OTHER], num_levels=0)
    assert (p["n_levels"], p["levels_off"], p["table_bytes"]) == (0, 480, 480 + 2 * 32)   # room for one level per job
    p = got_plan([(64, 65), OTHER])
    assert p["last_off"] == [64 * 6, 65 * 6, 64, 65, 64, 28, 3, 6]
    p = got_plan([(65, 64), OTHER])
    assert p["last_off"] == [65 * 6, 64 * 6, 65, 64, 64, 28, 6, 3]
    p = got_plan([(65, 65), OTHER])
    assert p["last_off"][4:] == [65, 56, 6, 6] and p["max_chunks"] == 4
    assert got_plan([(8192, 8192)])["max_rows_blocks"] == 2 and got_plan([(8193, 8192)])["max_rows_blocks"] == 3
    assert got_plan([(8192, 8193)])["max_dst_blocks"] == 2
    # the pinned block: 64 bytes for the counter, flags and states of 8 jobs, the tables, all 16-byte aligned
    p = got_plan([C1] * 5, uniform=1)
    assert (p["h_done_off"], p["h_state_off"], p["h_tables_off"]) == (64, 96, 96 + 8 * 392)
    assert p["pinned_bytes"] == 96 + 8 * 392 + 5 * 240 + 5 * 8 * 32
    for name in CASES:
        p = got_plan(**CASES[name])
        assert all(p[f] % 16 == 0 for f in ("h_done_off", "h_state_off", "h_tables_off", "levels_off", "table_bytes")), name
        assert p["h_done_off"] >= 64 and p["h_state_off"] - p["h_done_off"] >= 4 * p["state"]
        assert p["h_tables_off"] - p["h_state_off"] >= SIZEOF_STATE * p["state"] and p["state"] >= max(len(CASES[name]["jobs"]), 8)


def test_bad_arguments():
    f = lib().ppf_debug_icp_plan
    s, out = call_plan([C1])
    assert s == _capi.PPF_OK
    pin = IcpPlanIn()
    assert f(None, C.byref(out)) == _capi.PPF_ERR_INVALID and f(C.byref(pin), None) == _capi.PPF_ERR_INVALID
    bad = [dict(jobs=[]), dict(jobs=[C1] * 9), dict(jobs=[(0, 5)]), dict(jobs=[(5, 0)]), dict(jobs=[C1, (5, -1)]),
           dict(jobs=[C1], iterations=-1), dict(jobs=[C1], num_levels=-1), dict(jobs=[C1], num_levels=9),
           dict(jobs=[C1], tolerance=-1.0), dict(jobs=[C1], tolerance=float("nan")),
           dict(jobs=[C1, OTHER], uniform=1), dict(jobs=[C1, (C1[0], 5)], uniform=1)]
    for k in bad:
        s, out = call_plan(**k)
        assert s == _capi.PPF_ERR_INVALID, k
        assert "ppf_debug_icp_plan" in _capi.last_error() and bytes(out) == bytes(C.sizeof(IcpPlanOut)), k


def test_plan_struct_layouts_match_the_header(tmp_path):
    structs = [("ppf_debug_icp_plan_in", IcpPlanIn), ("ppf_debug_icp_plan_out", IcpPlanOut)]
    expr, got = [], []
    for cname, cls in structs:
        expr.append(f"sizeof({cname})")
        got.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            expr += [f"offsetof({cname}, {f})", f"sizeof((({cname}*)0)->{f})"]
            got += [getattr(cls, f).offset, getattr(cls, f).size]
    src = tmp_path / "icp_plan_sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ppf_hip.h"\nint main(){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "icp_plan_sz"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
