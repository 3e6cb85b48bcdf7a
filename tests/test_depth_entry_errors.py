"""The argument-error contract of the depth-image entries, byte for byte: every call of the table in
tests/golden/make_depth_entry_errors.py gives the status, the whole ppf_last_error() text and the cleared stats and outputs
that tests/golden/depth_entry_errors.json recorded before the stages shared one host front end -- including which error wins
when a call has two.  No GPU is needed.  Where there is one, the calls that passed every argument check when the file was
recorded (they ended in "no HIP device") are not made."""
import json
import os
import sys

import pytest

from conftest import GOLDEN
from yolo_ppf_pose_estimation_amd._capi import lib

sys.path.insert(0, GOLDEN)
import make_depth_entry_errors as M  # noqa: E402

with open(os.path.join(GOLDEN, "depth_entry_errors.json")) as f:
    WANT = json.load(f)
ENTRIES = ["ppf_cloud_from_depth", "ppf_cloud_from_depth_device", "ppf_cloud_from_depth_normals", "ppf_cloud_from_depth_normals_device",
           "ppf_depth_register", "ppf_depth_register_device", "ppf_depth_filter", "ppf_depth_filter_device", "ppf_depth_segments",
           "ppf_depth_segments_device", "ppf_depth_history_push", "ppf_depth_history_push_device", "ppf_depth_history_create"]


def test_the_fixture_holds_every_case_of_the_table():
    assert sorted(WANT) == sorted(ENTRIES)
    table = {}
    for entry, name, _ in M.cases():
        table.setdefault(entry, []).append(name)
    assert {e: sorted(v) for e, v in WANT.items()} == {e: sorted(v) for e, v in table.items()}
    assert all(M.VALID in WANT[e] and WANT[e][M.VALID][0] == "PPF_ERR_HIP" for e in ENTRIES if "register" not in e and "push" not in e)
    assert all(c[0] in ("PPF_ERR_INVALID", "PPF_ERR_HIP") for v in WANT.values() for c in v.values())


@pytest.mark.parametrize("entry", ENTRIES)
def test_statuses_texts_and_cleared_outputs_are_the_recorded_ones(entry):
    have_gpu = lib().ppf_device_count() > 0
    want = {n: c for n, c in WANT[entry].items() if not (have_gpu and c[0] == "PPF_ERR_HIP")}
    got = M.replay(lambda e, n: e == entry and n in want)
    assert len(want) >= 6 and sorted(got[entry]) == sorted(want)
    for name in want:
        assert got[entry][name] == want[name], (entry, name)
