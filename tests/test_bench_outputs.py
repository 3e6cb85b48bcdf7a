"""bench.py's plain run times the headline workload only (the other legs wait for --full), and --dump-outputs writes what the
last timed step computed: on the GPU, the C2 dump is the oracle's fixture (tests/golden/config_c2.npz)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from yolo_ppf_pose_estimation_amd import workloads as W
from yolo_ppf_pose_estimation_amd._capi import Pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_leaves_the_other_legs_to_full():
    plain = bench.parse_args(["--steps", "3"])
    assert plain.steps == 3 and not plain.full and plain.no_cpu_baseline and plain.no_other_configs
    full = bench.parse_args(["--full"])
    assert full.full and not full.no_cpu_baseline and not full.no_other_configs
    part = bench.parse_args(["--full", "--no-cpu-baseline"])
    assert part.no_cpu_baseline and not part.no_other_configs


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_pose_block_decodes_records_and_dump_is_float64(tmp_path, monkeypatch):
    import torch
    recs = (Pose * 3)()
    for i, r in enumerate(recs):
        r.pose[:] = [float(i * 16 + j) for j in range(16)]
        r.residual, r.model_index, r.num_votes = 0.5, i, 1000 + i
    words = np.frombuffer(bytes(recs), dtype=np.float64).reshape(3, C.sizeof(Pose) // 8)
    arrays = bench.pose_block_arrays(torch.from_numpy(words.copy()))
    np.testing.assert_array_equal(arrays["top_poses"], np.arange(48, dtype=np.float64).reshape(3, 4, 4))
    assert list(arrays["top_votes"]) == [1000, 1001, 1002] and list(arrays["top_model_index"]) == [0, 1, 2]
    bench.write_outputs(str(tmp_path / "out"), arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "out" / f"{k}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, v)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100)
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), arrays)


@pytest.mark.gpu
def test_plain_bench_dumps_the_oracle_result_of_c2(tmp_path):
    fx = np.load(os.path.join(ROOT, "tests", "golden", "config_c2.npz"))
    assert W.cloud_digest(W.c2_scene()) == str(fx["digest"])
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["cpu_baseline"] is None and not {"host_entry", "pipelined", "other_configs"} & set(line)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"top_poses", "top_votes", "top_model_index", "vote_triples", "raw_poses", "counters"}
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["vote_triples"], fx["triples"])
    np.testing.assert_array_equal(got["raw_poses"][::125], fx["raw_pose_first"])
    n_ref, n_poses, n_pairs, n_votes = got["counters"]
    assert (n_ref, n_poses, n_pairs, n_votes) == (2500, int(fx["n_final"][0]), int(fx["pairs"].sum()), int(fx["votes"].sum()))
    np.testing.assert_array_equal(got["top_votes"], fx["top_votes"])
    np.testing.assert_allclose(got["top_poses"], fx["top_poses"], rtol=0, atol=1e-9)
