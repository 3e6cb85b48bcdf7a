"""The C++ oracle's full accumulators against a second, independent statement of the voting specification
(tests/vote_oracle.py), on a case that is known to contain what the 6 x 8 toy case of test_oracle_kat.py meets only by luck:
a true `hash % slots` collision, a spill into the next model row, and a spill behind the last row."""
import numpy as np

import spill_scenes as S
import vote_oracle as V

SAMPLING = 0.15


def test_full_accumulators_equal_an_independent_numpy_voter(bottle):
    """Every cell of every reference point.  numpy's acos / atan2 / sin / cos stand where the oracle has its deterministic
    math: tests/golden/libm_tolerance.json records 0 of 2,500 triples differing between the two on a far larger case, and
    none differs here (seed 7)."""
    model, scene, ora, planted = S.second_source_case(bottle, SAMPLING)
    info = ora.info()
    voter = V.Voter(model, SAMPLING, info["num_angles"])
    assert (voter.slots, voter.dist_step, voter.angle_step) == (info["slots"], info["distance_step"], info["angle_step"])
    want = ora.match(scene, relative_scene_sample_step=1.0, presampled=True, cluster=False)
    assert want["n_ref"] == scene.shape[0]
    mixed = kept = dropped = 0
    for i in range(scene.shape[0]):
        acc, facts = voter.accumulator(scene, i)
        np.testing.assert_array_equal(acc, ora.accumulator(scene, i), err_msg=f"reference point {i}")
        assert facts["votes"] == int(want["votes_per_ref"][i])
        mixed += facts["mixed_buckets"]
        kept += facts["spills_kept"]
        dropped += facts["spills_dropped"]
        for ref, _, row in planted:
            if i == ref and row + 1 < info["n_ref"]:
                assert facts["spills_kept"] >= 1 and acc[row + 1, 0] >= 1
            if i == ref and row + 1 == info["n_ref"]:
                assert facts["spills_dropped"] >= 1
    assert mixed >= 1, "no voted bucket held model pairs of two different keys"    # (i)
    assert kept >= 1 and dropped >= 1                                             # (ii)


def test_the_planted_pairs_spill_by_the_oracle_alone(bottle):
    """The recount every spill test starts with (spill_scenes.Recount: ora.pairs(), O.pair_feature, O.alpha): the planted
    scene pair votes for its model row in bin numAngles, and the last row's such vote is not in the oracle's total."""
    model, scene, ora, planted = S.second_source_case(bottle, SAMPLING)
    rc = S.Recount(ora)
    want = ora.match(scene, relative_scene_sample_step=1.0, presampled=True, cluster=False)
    for ref, partner, row in planted:
        assert rc.spills(scene, ref, partner, row) >= 1
        inside, behind = rc.total(scene, ref)
        assert inside == int(want["votes_per_ref"][ref])
        if row == rc.N - 1:  # (the pairs share a bucket: the other planted reference point drops this row's vote too)
            assert behind >= 1
        if row + 1 < rc.N:
            assert ora.accumulator(scene, ref)[row + 1, 0] >= 1
