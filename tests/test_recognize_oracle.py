"""The numpy restatement of ppf_recognize_frame's specification (tests/recognize_oracle.py) against keys worked out by hand, its
invariants, and the conditions the stage was proposed under: does precision x recall over the quantised pair-feature keys name
the right model for one-sided, noisy views?  No GPU: the models are trained with the CPU oracle (OracleDetector).

The models of the recognition conditions are the four solids sampled at 0.05 of their diameter by recognize_cases.voxel_pick
(one untouched row per voxel) and trained presampled, 12-degree bins: 590 / 474 / 436 / 376 rows and 825 / 638 / 4,464 /
7,359 keys, the key counts the conditions were stated with.  12 seeded views a model with 4 degrees of normal noise and
0.5 mm of position noise, max_rows 400: the true model is first in 48 of 48, the runner-up at most 0.474 (box), 0.443
(cylinder), 0.213 (torus), 0.411 (bottle) of the winner; the bottle wins the reference crop with 0.334 against the torus's
0.238.  Seeds and noise are the first ones tried.

The sampler matters.  Trained from the full clouds, so that the detector's own samplePCByQuantization makes the rows (it
averages the normals of a voxel, which on the box's edges mixes two faces: 1,388 rows, 11,896 keys), the same views name
cylinder, torus and bottle in 36 of 36 (runner-up at most 0.798, 0.250, 0.742) but the box in 0 of 12: the cylinder wins
every box view, 0.084 .. 0.114 against 0.070 .. 0.094, at every noise level from none to 30 degrees.  DESIGN.md section 25
has the figures and what follows for a user."""
import math
import os

import numpy as np
import pytest

import oracle_lib as O
import recognize_cases as K
import recognize_oracle as R

INT32_MIN = -(2 ** 31)
A12 = (360.0 / 30.0) * math.pi / 180.0  # the angle step of 30 bins, as the table build computes it


def rows_of(*rows):
    return np.array(rows, dtype=np.float32)


def test_the_keys_of_a_hand_made_cloud():
    z, x = (0, 0, 1), (1, 0, 0)
    cloud = rows_of((0, 0, 0) + z, (0.1, 0, 0) + z, (0, 0.1, 0) + x, (0, 0, 0.2) + z)
    keys = R.quantise(R.pair_features(cloud), A12, 0.01)
    top = int(math.pi / A12)  # the bin of an angle of pi
    want = {(0, 1): (7, 7, 0, 10), (1, 0): (7, 7, 0, 10),            # along x, both normals across: 90 / 12 = 7.5
            (0, 3): (0, 0, 0, 20), (3, 0): (top, top, 0, 20),        # along both normals, and against them
            (0, 2): (7, 7, 7, 10), (2, 0): (7, 7, 7, 10),            # normals at a right angle, both across the line
            (1, 2): (7, 11, 7, 14), (2, 1): (3, 7, 7, 14),           # 135 / 12 = 11.25 and 45 / 12 = 3.75; 0.1414 / 0.01
            (1, 3): (2, 2, 0, 22), (3, 1): (12, 12, 0, 22),          # atan(1 / 2) = 26.57 degrees: 2.21; 153.43: 12.79; 0.2236 / 0.01
            (2, 3): (7, 2, 7, 22), (3, 2): (12, 7, 7, 22)}
    for (i, j), k in want.items():
        assert tuple(int(v) for v in keys[i, j]) == k, (i, j, keys[i, j], k)
    m = R.Model(cloud, A12, 0.01)
    assert [tuple(int(v) for v in k) for k in m.keys] == sorted(set(want.values())) and m.n_keys == 10
    assert (m.n_a, m.n_d) == (top + 2, 23)
    got = R.recognize([cloud], [m])[0]
    assert got["n_used"] == 4 and tuple(got["counts"][0]) == (12, 10) and tuple(got["scores"][0]) == (1.0, 1.0, 1.0)


def test_parallel_normals_give_the_int32_min_bin():
    n = (0.6, 0.8, 0.0)  # as float32 the dot product of this normal with itself is above 1: its acos is NaN
    cloud = rows_of((0, 0, 0) + n, (0, 0, 0.1) + n)
    assert float(np.sum(cloud[0, 3:6].astype(np.float64) ** 2)) > 1.0
    keys = R.quantise(R.pair_features(cloud), A12, 0.01)
    assert tuple(int(v) for v in keys[0, 1]) == (7, 7, INT32_MIN, 10) == tuple(int(v) for v in keys[1, 0])
    m = R.Model(cloud, A12, 0.01)
    assert m.keys.tolist() == [[7, 7, INT32_MIN, 10]]
    assert tuple(R.recognize([cloud], [m])[0]["counts"][0]) == (2, 1)  # a value like any other: it is known
    other = R.Model(rows_of((0, 0, 0, 0, 1, 0), (0, 0, 0.1, 0, 1, 0)), A12, 0.01)  # the same pair with an angle of exactly 0
    assert other.keys.tolist() == [[7, 7, 0, 10]] and tuple(R.recognize([cloud], [other])[0]["counts"][0]) == (0, 0)


def test_a_coincident_pair_has_the_zero_key_and_lexicographic_order_is_signed():
    cloud = rows_of((0.3, 0.2, 0.1, 0, 0, 1), (0.3, 0.2, 0.1, 1, 0, 0), (0.3, 0.2, 0.2, 0.6, 0.8, 0), (0.3, 0.2, 0.3, 0.6, 0.8, 0))
    keys = R.quantise(R.pair_features(cloud), A12, 0.01)
    assert keys[0, 1].tolist() == [0, 0, 0, 0] == keys[1, 0].tolist()  # the angles stay zero up to a distance of FLT_EPSILON
    m = R.Model(cloud, A12, 0.01)
    assert [tuple(k) for k in m.keys.tolist()] == sorted(tuple(k) for k in m.keys.tolist())
    assert any(k[2] == INT32_MIN for k in m.keys.tolist())


def test_the_stride_rule():
    cloud = np.arange(513 * 6, dtype=np.float32).reshape(513, 6)
    assert R.used_rows(cloud[:512], 512).shape[0] == 512                      # n = max_rows: every row
    u = R.used_rows(cloud, 512)                                               # n = max_rows + 1: every second row
    assert u.shape[0] == 257 and np.array_equal(u, cloud[::2])
    assert R.used_rows(cloud, 2).shape[0] == 2 and np.array_equal(R.used_rows(cloud, 2), cloud[::257])
    bad = cloud.copy()
    bad[2, 4] = np.nan
    bad[4, 0] = np.inf
    bad[3, :] = np.nan                                                        # not a candidate: nobody misses it
    assert np.array_equal(R.used_rows(bad, 512), np.delete(cloud[::2], [1, 2], axis=0))
    assert R.used_rows(np.zeros((0, 6), np.float32), 512).shape == (0, 6)
    got = R.recognize([None, np.zeros((0, 6), np.float32), cloud[:1]], [R.Model(cloud[:4], A12, 1.0)])
    assert [g["n_used"] for g in got] == [0, 0, 1] and [g["ranked"] for g in got] == [[], [], [0]]
    assert got[2]["scores"].tolist() == [[0.0, 0.0, 0.0]]                     # no pair: all three are 0


@pytest.fixture(scope="module")
def models():
    """the four models as the conditions name them: sampled at 0.05 of their diameter (one untouched row per voxel), 12-degree bins"""
    return [R.Model.from_detector(O.OracleDetector(0.05, 0.05, 30).train_model(K.voxel_pick(K.solid(k), 0.05), presampled=True))
            for k in K.KINDS]


def test_a_model_is_a_perfect_view_of_itself_and_no_far_pair_is_known(models):
    bottle = models[K.KINDS.index("bottle")]
    assert [m.n_keys for m in models] == [825, 638, 4464, 7359]
    got = R.recognize([bottle.rows], [bottle], max_rows=2048)[0]
    n = bottle.rows.shape[0]
    assert got["n_used"] == n and tuple(got["counts"][0]) == (n * (n - 1), bottle.n_keys)
    assert tuple(got["scores"][0]) == (1.0, 1.0, 1.0)
    span = float(np.linalg.norm(bottle.rows[:, :3].max(axis=0) - bottle.rows[:, :3].min(axis=0)))
    far = rows_of((0, 0, 0, 0, 0, 1), (0, 0, 1.5 * span, 0, 0, 1), (1.5 * span, 0, 0, 0, 0, 1))
    for m in models:
        assert tuple(R.recognize([far], [m])[0]["counts"][0]) == (0, 0)


@pytest.mark.parametrize("kind", K.KINDS)
def test_the_recognition_conditions(models, kind):
    """12 seeded one-sided views of each model: the true model first, the runner-up at most 0.85 of it (the module's docstring
    has the figures)"""
    ki = K.KINDS.index(kind)
    full = K.solid(kind)
    worst = 0.0
    for v in range(12):
        got = R.recognize([K.one_sided_view(full, 1000 * ki + v, normal_deg=4.0, pos_sigma=0.0005)], models, max_rows=400, top=2)[0]
        assert 0 < got["n_used"] <= 400
        n_pairs = got["n_used"] * (got["n_used"] - 1)
        for m, (known, hit) in enumerate(got["counts"]):
            assert known <= n_pairs and hit <= models[m].n_keys and hit <= known
        s = got["scores"][:, 2]
        print(kind, v, got["n_used"], np.round(s, 4).tolist(), got["ranked"])
        assert got["ranked"][0] == ki, (kind, v, s.tolist())
        worst = max(worst, float(s[got["ranked"][1]] / s[ki]))
    print(kind, "runner-up at most", round(worst, 3))
    assert worst <= 0.85, (kind, worst)


def test_the_bottle_wins_the_reference_crop(models):
    crop = np.load(os.path.join(K.GOLDEN, "c1_crop_xyzn.npy"))
    got = R.recognize([crop], models, max_rows=512, top=4)[0]
    print(got["n_used"], got["scores"].tolist(), got["ranked"])
    assert got["ranked"][0] == K.KINDS.index("bottle"), got["scores"].tolist()
