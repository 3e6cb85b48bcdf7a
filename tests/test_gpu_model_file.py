"""tests/golden/tiny_model.ppf on the device: training its cloud again gives the file byte for byte (training proved
deterministic when the fixture was made: two trainings gave equal bytes), loading it and saving it again does too, and the
loaded model votes like the trained one -- the group records a loader derives from the file's table on the host are the
ones training derives from the device's."""
import numpy as np
import pytest

import test_model_file as M
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture_bytes():
    with open(M.FIXTURE, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def trained():
    return PPF3DDetector(M.SAMPLING, M.DISTANCE, max_tile_refs=M.MAX_TILE_REFS).trainModel(M.tiny_cloud(), presampled=True)


@pytest.fixture(scope="module")
def loaded(fixture_bytes):
    return PPF3DDetector(M.SAMPLING, M.DISTANCE).from_bytes(fixture_bytes)


def test_training_the_fixture_cloud_gives_the_committed_bytes(trained, fixture_bytes):
    assert trained.to_bytes() == fixture_bytes


def test_load_then_save_is_the_identity(loaded, fixture_bytes, tmp_path):
    assert loaded.to_bytes() == fixture_bytes
    loaded.write(str(tmp_path / "again.ppf"))
    assert (tmp_path / "again.ppf").read_bytes() == fixture_bytes
    assert loaded.info() == PPF3DDetector().read(str(tmp_path / "again.ppf")).info()


def test_loaded_and_trained_model_vote_alike(trained, loaded):
    """The scene is the model's own cloud, moved: every reference point hits the planar grid's few big buckets often enough
    for count tables, so the votes go through the group records of both models."""
    assert trained.info() == loaded.info()
    c, s = np.cos(0.7), np.sin(0.7)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, 0.8, -0.6], [0.0, 0.6, 0.8]])
    cloud = M.tiny_cloud().astype(np.float64)
    between = cloud[:64] + [0.005, 0.005, 0.0, 0.0, 0.0, 0.0]  # the grid again, half a cell on: twice the hits per bucket
    cloud = np.concatenate([cloud, between])
    scene = np.ascontiguousarray(np.concatenate([cloud[:, :3] @ R.T + [0.02, -0.01, 0.3], cloud[:, 3:] @ R.T], 1), dtype=np.float32)
    a = trained.raw_votes(scene, 1.0, 0.05, presampled=True)
    b = loaded.raw_votes(scene, 1.0, 0.05, presampled=True)
    assert a["n_ref"] == b["n_ref"] == scene.shape[0]
    assert a["stats"]["n_tables"] > 0 and a["stats"]["n_tables"] == b["stats"]["n_tables"]
    assert a["stats"]["n_votes"] == b["stats"]["n_votes"] > 0
    np.testing.assert_array_equal(a["triples"], b["triples"])
