"""Full accumulators, cell by cell, on every voting path of k_vote: direct items and count tables, 16- and 32-bit cells, the
re-vote after a 16-bit overflow, one tile and several, staging segments, group rounds and batches of reference points, calls
repeated after a pool ran out, warm workspaces, other alpha resolutions, match_S2B and non-finite scene rows.

The dump runs on the caller's workspace (Workspace.accumulators -> ppf_debug_accumulators_ws), so the workspace options that
select those paths apply.  `check` ties every dump to the same call's product outputs: its sum is the call's vote counter and
its first maximum is the call's vote triple.

The scenes hold planted pairs whose alpha bin is numAngles (tests/spill_scenes.py): the vote that counts in the next model
row's bin 0.  They sit where the accumulator layout is irregular: the last low-half row of a tile (H - 1 -> H: 16-bit cells
keep that vote in the word behind the rows, 32-bit cells in the other half-pass's workgroup), the last row of a tile (the
next tile's first cell) and the model's last row (dropped).  Every spill is first confirmed by a recount with the oracle's
pair table and feature functions alone."""
import numpy as np
import pytest

import oracle_lib as O
import spill_scenes as S
import vote_oracle as V
from test_gpu_sparse_tables import MIN_HITS, Rings, sector
from yolo_ppf_pose_estimation_amd import _capi, synth
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
from yolo_ppf_pose_estimation_amd.device import Workspace

pytestmark = pytest.mark.gpu

SAMPLING, DISTANCE = 0.08, 0.05  # the bottle at 430 rows
N_SCENE, REF_STRIDE = 3000, 200  # 15 reference points per dump: rows 0, 200, ..., 2800
A_REF, RING_HITS = 5, 955        # the model row the ring of the scene is built around: a run of five count tables in a big bucket,
                                 # which saves more atomics than the padding of all the direct items of a call costs (ten tiles: most)
TILINGS = [0, 150, 43]           # max_tile_refs: one tile of 430 rows (even, H = 215); 144 + 144 + 142; ten tiles of 43 (odd, H = 22 > 21)


def check(ws, det, ora, scene, step, refs, want=None, **kw):
    """Dump the accumulators of one call on `ws` and compare, for every reference point (scene rows `refs`): (a) every cell with
    the oracle's accumulator, (b) the sum with the call's votes_per_ref, (c) the first maximum with the call's vote triple.
    `want` caches the oracle's accumulators per scene row.  Returns the call's statistics."""
    acc = ws.accumulators(det, scene, step, **kw)
    res = ws.results(scene.shape[0])
    votes, _ = ws.ref_counters(max(res["n_ref"], 1))
    assert acc.shape[0] == res["n_ref"] == len(refs)
    A = acc.shape[2]
    want = {} if want is None else want
    for k, i in enumerate(refs):
        if i not in want:
            want[i] = ora.accumulator(scene, i, sampled_paired=kw.get("edge"))
        np.testing.assert_array_equal(acc[k], want[i], err_msg=f"reference point {i} (dumped as {k})")
        assert int(acc[k].sum(dtype=np.uint64)) == int(votes[k]), f"reference point {i}: the dump's sum is not the call's counter"
        flat = acc[k].reshape(-1)
        j = int(np.argmax(flat))
        assert (j // A, j % A, int(flat[j])) == tuple(int(v) for v in res["triples"][k]), f"reference point {i}: triple"
    return res["stats"]


def rings_of(ora):
    """test_gpu_sparse_tables.Rings on an oracle that is already trained (there: on the bottle)."""
    r = Rings.__new__(Rings)
    r.ora, r.info = ora, ora.info()
    r.A, r.model = r.info["num_angles"], ora.sampled_model().astype(np.float64)
    n = r.info["n_ref"]
    r.hsh = ora.pairs()[0]
    u, c = np.unique(r.hsh[~np.eye(n, dtype=bool)], return_counts=True)
    r.bucket_size = dict(zip(u.tolist(), c.tolist()))
    return r


class Case:
    """One tiling / alpha resolution of the 430-row bottle with spill pairs planted for that tiling, its detector and oracle,
    and the 3,000-row scene: the planted pairs at reference points 200, 400, ..., a ring of 955 hits around row 1000."""

    def __init__(self, bottle, rows, max_tile_refs, num_angles):
        plain = PPF3DDetector(SAMPLING, DISTANCE, num_angles, max_tile_refs=max_tile_refs).trainModel(rows, presampled=True).info()
        self.N, self.T, self.n_tiles = plain["n_ref"], plain["tile_refs"], plain["n_tiles"]
        self.H = (self.T + 1) // 2
        a_rows = [self.H - 1]                                        # the last low-half row of tile 0
        if self.n_tiles > 1:
            a_rows += [self.T - 1,                                   # the last row of tile 0
                       (self.n_tiles - 1) * self.T + self.H - 1]     # the half boundary of the last (possibly shorter) tile
            assert a_rows[-1] + 1 < self.N
        a_rows.append(self.N - 1)                                    # the model's last row: its spill is dropped
        free = [r for r in range(10, self.N) if r not in a_rows and r != A_REF]
        self.pairs = list(zip(a_rows, free))
        self.model = S.plant(rows, self.pairs)
        self.det = PPF3DDetector(SAMPLING, DISTANCE, num_angles, max_tile_refs=max_tile_refs).trainModel(self.model, presampled=True)
        self.ora = O.OracleDetector(SAMPLING, DISTANCE, num_angles=num_angles).train_model(self.model, presampled=True)
        info = self.det.info()
        assert (info["n_ref"], info["tile_refs"], info["n_tiles"]) == (self.N, self.T, self.n_tiles)
        assert info["num_angles"] == self.ora.info()["num_angles"] == num_angles
        self.A = num_angles
        self.rc = S.Recount(self.ora)
        rings = rings_of(self.ora)
        scene = synth.make_scene(bottle, n_points=N_SCENE, seed=31)[0].astype(np.float32)
        self.planted = []
        for k, (a, b) in enumerate(self.pairs):
            ref = REF_STRIDE * (k + 1)
            scene[ref], scene[ref + 1] = S.scene_rows(self.model, a, b)
            self.planted.append((ref, ref + 1, a))
        self.ring_ref = 1000
        for lo in (5000, 2000, 1000):  # the partner of the biggest bucket that has one (a tenth of a bin from every bin edge)
            try:
                partner = rings.partners(A_REF, lo=lo, hi=10 ** 6, margin=0.1)[0]
                break
            except AssertionError:
                assert lo > 1000
        ring = rings.ring(A_REF, partner, sector(40.0, RING_HITS)).astype(np.float32)
        scene[self.ring_ref] = self.model[A_REF]
        self.ring_rows = [r for r in range(self.ring_ref + 1, N_SCENE) if r % REF_STRIDE > 1][:RING_HITS]
        scene[self.ring_rows] = ring
        self.scene = scene
        self.refs = list(range(0, N_SCENE, REF_STRIDE))
        self.want = {}        # oracle accumulators by scene row, computed once
        self._spills_ok = False

    def assert_spills(self, scene=None, paired=None):
        """By the oracle alone: every planted scene pair casts at least one vote of its model row into bin numAngles; the last
        row's lies behind the buffer and is not part of the oracle's total."""
        if scene is None and self._spills_ok:
            return
        sc = self.scene if scene is None else scene
        partner = (lambda row: row) if paired is None else (lambda row: int(np.flatnonzero((paired == sc[row]).all(axis=1))[0]))
        for ref, part, row in self.planted:
            assert self.rc.spills(sc, ref, partner(part), row, paired) >= 1, f"no spill out of model row {row}"
            if row == self.N - 1:
                inside, behind = self.rc.total(sc, ref, paired)
                assert behind >= 1
                assert inside == int(self.ora.accumulator(sc, ref, sampled_paired=paired).sum(dtype=np.uint64))
            else:
                assert self.ora.accumulator(sc, ref, sampled_paired=paired)[row + 1, 0] >= 1
        # the ring is a run that reaches the count tables
        runs = rings_of(self.ora).runs_of(sc, self.ring_ref) if paired is None else None
        assert runs is None or max(len(v) for v in runs.values()) >= RING_HITS >= MIN_HITS
        if scene is None:
            self._spills_ok = True

    def run(self, ws, mode, **kw):
        return check(ws, self.det, self.ora, self.scene, 1.0, self.refs, self.want, ref_stride=REF_STRIDE, vote_mode=mode, **kw)


def tables_fired(st, mode, expect=True):
    """vote_mode 0: count tables were built and saved atomics; vote_mode 1 (or an alpha resolution beyond the tables'): none."""
    if mode == 0 and expect:
        assert st["n_tables"] > 0 and st["n_lds_atomics"] < st["n_votes"]
    else:
        assert st["n_tables"] == 0


@pytest.fixture(scope="module")
def rows(bottle):
    return O.OracleDetector(SAMPLING, DISTANCE).train_model(bottle).sampled_model()


@pytest.fixture(scope="module")
def cases(bottle, rows):
    made = {}

    def get(max_tile_refs=0, num_angles=30):
        key = (max_tile_refs, num_angles)
        if key not in made:
            made[key] = Case(bottle, rows, max_tile_refs, num_angles)
        return made[key]
    return get


def test_the_tilings_have_even_and_odd_tiles_and_unequal_halves(cases):
    shapes = [(cases(t).n_tiles, cases(t).T, cases(t).N - (cases(t).n_tiles - 1) * cases(t).T) for t in TILINGS]
    assert shapes == [(1, 430, 430), (3, 144, 142), (10, 43, 43)]
    assert cases(150).H == 72 and 142 - 72 != 72 and cases(43).H == 22 != 43 - 22


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("tiling", TILINGS)
def test_32_bit_cells(cases, tiling, mode):
    """PPF_OPT_ACC32 = 1: every (reference point, tile) in two half-passes; the spill out of row H - 1 is what one half owes the
    other (k_finalize and the dump add it to row H, bin 0)."""
    c = cases(tiling)
    c.assert_spills()
    ws = Workspace()
    ws.set_option(_capi.PPF_OPT_ACC32, 1)
    st = c.run(ws, mode)
    assert st["n_acc32_items"] == len(c.refs) * c.n_tiles and st["n_retries"] == 0
    tables_fired(st, mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("tiling", TILINGS)
def test_default_cells(cases, tiling, mode):
    """16-bit cells, two model rows per word: the spill out of row H - 1 lives in the low half of the word behind the rows,
    the one out of a tile's last row in the next tile's first cell."""
    c = cases(tiling)
    c.assert_spills()
    ws = Workspace()
    st = c.run(ws, mode)
    assert st["n_acc32_items"] == 0 and st["n_retries"] == 0
    tables_fired(st, mode)
    again = c.run(ws, mode)  # the warm workspace: pools sized from what the first call saw
    assert again["n_retries"] == 0 and again["n_acc32_items"] == 0 and again["n_votes"] == st["n_votes"]


# ---- the re-vote after a 16-bit overflow -----------------------------------------------------------------------------------
def _plane(uv):
    """Points (0, u, v) of the plane x = 0 with the normal (1, 0, 0): every frame is the identity."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    return np.hstack([np.zeros((uv.shape[0], 1)), uv, np.tile([1.0, 0.0, 0.0], (uv.shape[0], 1))]).astype(np.float32)


def _far(rng, n):
    return _plane(np.array([0.1, 0.02]) + rng.uniform(-5e-4, 5e-4, size=(n, 2)))


ORIGIN = _plane([[0.0, 0.0]])
PARTNER = _plane([[-S.D, 0.0]])  # the origin's spill partner: alpha_m = (float)pi


def _around_the_half_boundary(body):
    """Model rows with the origin at row H - 1 (H = half the rows of the one tile, rounded up) and its partner before it: the
    origin's spill counts in row H, bin 0 -- the cell the dump clears after a 16-bit overflow and the 32-bit launch re-adds."""
    n = body.shape[0] + 2
    h = (n + 1) // 2
    return np.vstack([body[:h - 2], PARTNER, ORIGIN, body[h - 2:]]).astype(np.float32), h


def _lifted_partner():
    return S.scene_rows(np.vstack([ORIGIN, PARTNER]), 0, 1)[1]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n_far", [199, 200])
def test_a_cell_beyond_65535_votes_is_voted_again(n_far, mode):
    """The spot of test_gpu_robustness (1,000 scene points in one spot seen from the reference point, 200 model points in the same
    spot seen from a model point: about 200,000 votes in one cell), laid into the plane x = 0 so that a spill pair fits, with
    241 and 242 model rows.  Cold workspace: flagged and voted again with 32-bit cells; warm: 32-bit cells from the start."""
    rng = np.random.default_rng(3)
    model, H = _around_the_half_boundary(np.vstack([_far(rng, n_far), _plane(rng.uniform(-0.1, 0.1, size=(40, 2)))]))
    scene = np.vstack([ORIGIN, _lifted_partner()[None, :], _far(rng, 1000), _plane(rng.uniform(-0.1, 0.1, size=(40, 2)))]).astype(np.float32)
    assert model.shape[0] == n_far + 42 and (model[H - 1] == ORIGIN[0]).all()
    det = PPF3DDetector(0.05, 0.05).trainModel(model, presampled=True)
    ora = O.OracleDetector(0.05, 0.05).train_model(model, presampled=True)
    info = det.info()
    assert (info["n_tiles"], info["tile_refs"]) == (1, model.shape[0]) and info["tile_refs"] > H
    assert S.Recount(ora).spills(scene, 0, 1, H - 1) >= 1
    want = {0: ora.accumulator(scene, 0)}
    assert want[0].max() > 65535 and want[0][H, 0] >= 1
    step = 1.0 / scene.shape[0]  # one reference point: row 0
    ws = Workspace()
    for _ in range(2):
        st = check(ws, det, ora, scene, step, [0], want, vote_mode=mode)
        assert st["n_retries"] == 0 and st["n_acc32_items"] == 1


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n_far", [298, 299])
def test_a_few_overflowing_reference_points_among_others(bottle, rows, n_far, mode):
    """The spot glued onto the bottle (730 and 731 model rows) and onto an ordinary crop, whose other reference points see
    nothing of it: the reference point at the origin overflows its 16-bit cells and is voted again, the others keep their
    16-bit result.  Its votes are more than a tenth of the call's, so the warm workspace votes every item with 32-bit cells."""
    rng = np.random.default_rng(4)
    model, H = _around_the_half_boundary(np.vstack([_far(rng, n_far), rows]))
    scene = synth.make_scene(bottle, n_points=N_SCENE, seed=5)[0].astype(np.float32)
    scene[0], scene[1] = ORIGIN[0], _lifted_partner()
    spot = [r for r in range(2, N_SCENE) if r % REF_STRIDE][:1200]
    scene[spot] = _far(rng, len(spot))
    det = PPF3DDetector(SAMPLING, DISTANCE).trainModel(model, presampled=True)
    ora = O.OracleDetector(SAMPLING, DISTANCE).train_model(model, presampled=True)
    info = det.info()
    assert (info["n_tiles"], info["tile_refs"]) == (1, model.shape[0]) and info["tile_refs"] > H
    assert S.Recount(ora).spills(scene, 0, 1, H - 1) >= 1
    refs = list(range(0, N_SCENE, REF_STRIDE))
    want = {i: ora.accumulator(scene, i) for i in refs}
    over = [i for i in refs if want[i].max() > 65535]
    assert over == [0] and want[0][H, 0] >= 1
    share = int(want[0].sum(dtype=np.uint64)) / sum(int(want[i].sum(dtype=np.uint64)) for i in refs)
    assert share > 0.1  # twice the twentieth of a call's votes at which a workspace switches to 32-bit cells
    ws = Workspace()
    st = check(ws, det, ora, scene, 1.0, refs, want, ref_stride=REF_STRIDE, vote_mode=mode)
    assert len(refs) > st["n_acc32_items"] >= len(over) and st["n_retries"] == 0
    st = check(ws, det, ora, scene, 1.0, refs, want, ref_stride=REF_STRIDE, vote_mode=mode)
    assert st["n_acc32_items"] == len(refs) and st["n_retries"] == 0


# ---- staging segments, group rounds, batches ------------------------------------------------------------------------------
ROUND_BUCKETS, BATCH_REFS = 500, 4


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("knobs", ["staging", "rounds", "batches", "all"])
def test_staging_segments_group_rounds_and_batches(cases, knobs, mode):
    c = cases(150)
    c.assert_spills()
    ws = Workspace()
    if knobs in ("staging", "all"):
        ws.set_option(_capi.PPF_OPT_RUN_STAGING, 64)
    if knobs in ("rounds", "all"):
        ws.set_option(_capi.PPF_OPT_GROUP_ROUND_BUCKETS, ROUND_BUCKETS)
        assert c.det.info()["n_buckets"] > 3 * ROUND_BUCKETS
    if knobs in ("batches", "all"):
        ws.set_option(_capi.PPF_OPT_BATCH_REFS, BATCH_REFS)
    st = c.run(ws, mode)
    assert st["n_batches"] == (-(-len(c.refs) // BATCH_REFS) if knobs in ("batches", "all") else 1)
    assert -(-len(c.refs) // BATCH_REFS) >= 3
    tables_fired(st, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_pools_that_start_too_small(cases, mode):
    """The call is repeated with bigger pools (the dump starts from zeros each time); the same workspace then runs once."""
    c = cases(0)
    c.assert_spills()
    ws = Workspace()
    ws.set_option(_capi.PPF_OPT_HIT_FRACTION, 0.002)
    ws.set_option(_capi.PPF_OPT_TABLE_FRACTION, 1e-6)
    st = c.run(ws, mode)
    assert st["n_retries"] >= 1
    tables_fired(st, mode)
    again = c.run(ws, mode)
    assert again["n_retries"] == 0 and again["n_votes"] == st["n_votes"]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("num_angles", [12, 31, 36])
def test_alpha_resolutions(cases, num_angles, mode):
    """12 and 31 bins (the most the count tables take) and 36 (direct votes only).  The spill does not depend on the resolution:
    alpha_m - alpha_s is 2 pi and a little."""
    c = cases(0, num_angles)
    c.assert_spills()
    st = c.run(Workspace(), mode)
    tables_fired(st, mode, expect=num_angles <= 31)


@pytest.mark.parametrize("mode", [0, 1])
def test_s2b_with_an_edge_cloud_that_differs_from_the_scene(cases, mode):
    c = cases(150)
    keep = np.arange(N_SCENE) % 5 == 1
    keep[[part for _, part, _ in c.planted]] = True
    keep[c.ring_rows] = True
    edge = np.ascontiguousarray(c.scene[keep])
    assert edge.shape[0] < N_SCENE // 2
    c.assert_spills(c.scene, edge)
    st = check(Workspace(), c.det, c.ora, c.scene, 1.0, c.refs, {}, ref_stride=REF_STRIDE, vote_mode=mode, edge=edge)
    assert st["n_paired"] == edge.shape[0]
    tables_fired(st, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_non_finite_scene_rows(cases, mode):
    """A few rows with a NaN or an infinity: the batch goes through k_group's checking path."""
    c = cases(150)
    scene = c.scene.copy()
    for row, col, v in [(7, 0, np.nan), (450, 4, np.inf), (2103, 2, -np.inf), (2222, 5, np.nan), (2999, 1, np.inf)]:
        assert row not in c.refs and row != c.ring_ref and row not in c.ring_rows and row not in [p for _, p, _ in c.planted]
        scene[row, col] = v
    for ref, part, row in c.planted:
        assert c.rc.spills(scene, ref, part, row) >= 1
    st = check(Workspace(), c.det, c.ora, scene, 1.0, c.refs, {}, ref_stride=REF_STRIDE, vote_mode=mode)
    tables_fired(st, mode)


# ---- the second source ------------------------------------------------------------------------------------------------------
def test_device_accumulators_equal_the_independent_voter(bottle):
    """The case of tests/test_vote_oracle.py (about 120 model rows, 400 reference points, a kept and a dropped spill), the
    device's dump against tests/vote_oracle.py directly: the C++ oracle is not involved."""
    model, scene, ora, planted = S.second_source_case(bottle)
    det = PPF3DDetector(0.15, 0.05).trainModel(model, presampled=True)
    voter = V.Voter(model, 0.15, det.info()["num_angles"])
    assert (voter.slots, voter.dist_step) == (det.info()["slots"], det.info()["distance_step"])
    ws = Workspace()
    acc = ws.accumulators(det, scene, 1.0)
    votes, _ = ws.ref_counters(scene.shape[0])
    assert acc.shape[0] == scene.shape[0]
    kept = dropped = 0
    for i in range(scene.shape[0]):
        want, facts = voter.accumulator(scene, i)
        np.testing.assert_array_equal(acc[i], want, err_msg=f"reference point {i}")
        assert facts["votes"] == int(votes[i])
        kept, dropped = kept + facts["spills_kept"], dropped + facts["spills_dropped"]
    assert kept >= 1 and dropped >= 1
