"""Group records: the entries of a (tile, bucket) that share accumulator row and count-table shift X cast their counted adds
from one merged record of up to four cells when the table is narrow (largest count <= 63); a wide table votes entry by entry.

Every scene is first confirmed on the CPU alone (oracle.pairs() and the oracle's features): that the visited bucket holds the
group sizes, the guard-band entry or the number of chunks the case is about, and that the table's largest count is what it
should be.  Then the device's full accumulators are compared with the oracle's cell by cell and the dump's sum with the call's
counter (`check` of test_gpu_accumulators), and no 16-bit cell may have been voted again: a group record that loses or doubles
an entry changes the votes found against the votes issued, which shows as a re-vote with 32-bit cells that mends the result."""
import math

import numpy as np
import pytest

import oracle_lib as O
import spill_scenes as S
from test_gpu_accumulators import (ORIGIN, REF_STRIDE, TILINGS, Case, _around_the_half_boundary, _far, _lifted_partner, _plane,
                                   check)
from test_gpu_sparse_tables import MIN_HITS, Rings, columns, sector, spread
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
from yolo_ppf_pose_estimation_amd.device import Workspace

pytestmark = pytest.mark.gpu

SAMPLING, DISTANCE = 0.08, 0.05   # the bottle at 430 rows: one tile
AGG_Q, AGG_SUB = 64, 191          # cells per alpha bin, hits per count table
GROUP_CELLS, NARROW_MAX = 4, 63   # cells per group record; the largest count of a table whose rows add up four to a byte
AGG_CHUNK, VOTE_CHUNK = 1024, 1024  # pair records per count-table item / per direct item
MIN_RECORDS = 32                  # a (tile, bucket) of fewer pair records votes directly


def records_for(entries):
    """Pair records of a (tile, bucket) of that many entries (dealing position j = record 32*(j/64) + j%32)."""
    return 32 * (entries // 64) + min(32, entries % 64)


class Groups(Rings):
    """Rings plus the (row, X) groups of a bucket, from oracle.pairs() alone."""

    def __init__(self, bottle):
        super().__init__(bottle)
        self.alp = self.ora.pairs()[1]
        self.off = ~np.eye(self.info["n_ref"], dtype=bool)

    def entries(self, h):
        """(row, X, alpha_m) of the entries of bucket h; X = floor(alpha_m * A / (4 pi) + A / 2) in fp32, as the table build has it."""
        i, j = np.nonzero((self.hsh == h) & self.off)
        am = self.alp[i, j].astype(np.float32)
        x = am * np.float32(self.A / (4 * math.pi)) + np.float32(0.5 * self.A)
        return i, np.floor(x).astype(np.int64), am

    def group_sizes(self, h):
        i, X, _ = self.entries(h)
        return np.unique(i * 64 + X, return_counts=True)[1]

    def group_records(self, h):
        """Group records of the real entries of bucket h: a group of g entries makes ceil(g / 4)."""
        return int(np.sum((self.group_sizes(h) + GROUP_CELLS - 1) // GROUP_CELLS))

    def pair_in(self, h, margin=0.2):
        """A model pair (a, b) of bucket h that scenes can be built around (Rings.partners)."""
        size = self.bucket_size[h]
        for a in np.unique(np.nonzero((self.hsh == h) & self.off)[0]).tolist():
            try:
                b = self.partners(a, lo=size, hi=size, margin=margin)[0]
            except AssertionError:
                continue
            if int(self.hsh[a, b]) == h:
                return a, b
        return None


@pytest.fixture(scope="module")
def groups(bottle):
    return Groups(bottle)


@pytest.fixture(scope="module")
def det(bottle):
    return PPF3DDetector(SAMPLING, DISTANCE).trainModel(bottle)


@pytest.fixture(scope="module")
def mixed(groups):
    """(a) The biggest bucket of the 430-row model whose entries form groups of 1, 2, 3, 4 and at least 5 entries and that a
    scene can be built around: (bucket, a, b)."""
    for h, size in sorted(groups.bucket_size.items(), key=lambda kv: -kv[1]):
        if size < 4 * 64 * 2:  # several blocks of 64 pair records, so that fewer group records are fewer blocks
            break
        g = groups.group_sizes(h)
        if {1, 2, 3, 4} <= set(g.tolist()) and g.max() >= 5:
            pair = groups.pair_in(h)
            if pair:
                return (h,) + pair
    pytest.fail("no bucket of the 430-row model has groups of 1, 2, 3, 4 and >= 5 entries")


def hits_of(groups, scene, h):
    """By the oracle alone: alpha_s of the hits of reference point 0 in bucket h, in scene order; the scene has no other run."""
    al = []
    for k in range(1, scene.shape[0]):
        _, _, hk = groups.feature(scene[0, :3], scene[0, 3:], scene[k, :3], scene[k, 3:])
        if hk in groups.bucket_size:
            assert hk == h, "the scene has a second run"
            al.append(O.alpha(scene[0, :3], scene[0, 3:], scene[k, :3]))
    return np.array(al)


def largest_count(alphas, A):
    """Largest count of the table of these hits: T[q][j] = hits with cell < q and Y + 8 == j plus hits with cell > q and
    Y + 8 == j - 1, over the cells q < 64 and the columns j <= 16."""
    x = np.asarray(alphas, dtype=np.float64) * (A / (4 * math.pi))
    Y = np.floor(x).astype(np.int64) + 8
    p = np.minimum(np.floor((x - np.floor(x)) * AGG_Q).astype(np.int64), AGG_Q - 1)
    best = 0
    for q in range(AGG_Q):
        for j in range(17):
            best = max(best, int(np.sum((p < q) & (Y == j)) + np.sum((p > q) & (Y == j - 1))))
    return best


def ring_scene(groups, a, b, alphas):
    return groups.scene(a, [groups.ring(a, b, alphas)])


def run_one(det, ora, scene, mode=0, ws=None, acc32=None):
    """One reference point (scene row 0), checked cell by cell; 16-bit cells must not have been voted again."""
    ws = Workspace() if ws is None else ws
    if acc32 is not None:
        ws.set_option(_capi.PPF_OPT_ACC32, acc32)
    st = check(ws, det, ora, scene, 1.0, [0], {}, ref_offset=0, ref_stride=scene.shape[0], vote_mode=mode)
    assert st["n_retries"] == 0
    if acc32 is None:
        assert st["n_acc32_items"] == 0, "votes found differ from votes issued: a 16-bit item was voted again"
    return st


# ---- (a) group sizes, (f) atomic counts -------------------------------------------------------------------------------------
def test_a_bucket_with_groups_of_one_to_five_and_more(groups, det, mixed):
    h, a, b = mixed
    g = groups.group_sizes(h)
    assert {1, 2, 3, 4} <= set(g.tolist()) and g.max() >= 5
    # (e) more than one chunk of 1,024 pair records: every table of the run is voted by several items, each with a slice of
    # the bucket's group records (bucket 1995723043 of the 430-row bottle: 4,308 entries, 2,164 records, three chunks)
    assert records_for(groups.bucket_size[h]) > AGG_CHUNK >= MIN_RECORDS
    for alphas in (sector(40.0, 48), spread(MIN_HITS), spread(AGG_SUB)):
        scene = ring_scene(groups, a, b, alphas)
        al = hits_of(groups, scene, h)
        assert len(al) == len(alphas) >= MIN_HITS and largest_count(al, groups.A) <= NARROW_MAX
        st = run_one(det, groups.ora, scene)
        assert st["n_tables"] == 1
        run_one(det, groups.ora, scene, mode=1)


def test_atomic_counts_of_the_mixed_bucket(groups, det, mixed):
    """(f) One run of 48 hits over the whole circle (every column set, a narrow table) on the bucket of (a).  The per-entry
    scheme casts 2 x 17 counted lane-operations for every block of 64 pair records and then the own-cell votes; the merged one
    casts the same per block of 64 GROUP records and no more own-cell votes (lanes past the end cast none): with fewer blocks
    its total is below the per-entry scheme's counted part alone.  Direct votes: 2 x 64 per block of 64 records and hit, per
    chunk of 1,024 records -- the parent's formula."""
    h, a, b = mixed
    scene = ring_scene(groups, a, b, spread(48))
    al = hits_of(groups, scene, h)
    ys = (np.floor(al * groups.A / (4 * math.pi)).astype(np.int64) + 8).tolist()
    assert len(al) == 48 and columns(ys) == 0x1FFFF and largest_count(al, groups.A) <= NARROW_MAX
    entries = groups.bucket_size[h]
    c = records_for(entries)
    chunks = [min(AGG_CHUNK, c - k) for k in range(0, c, AGG_CHUNK)]
    blocks = sum(-(-ck // 64) for ck in chunks)
    # group records of the real entries plus, at most, one per padding slot of the bucket's last records; every chunk's slice
    # may end with a block that is not full
    g_blocks = -(-records_for(groups.group_records(h) + 2 * c - entries) // 64) + len(chunks)
    assert g_blocks < blocks, "the bucket's group records fill as many blocks as its entries"
    per_entry_counted = 2 * 17 * 64 * blocks
    st = run_one(det, groups.ora, scene)
    assert st["n_tables"] == 1
    assert st["n_lds_atomics"] < per_entry_counted
    assert st["n_lds_atomics"] >= 2 * 17 * 64 * -(-records_for(groups.group_records(h)) // 64)
    direct = run_one(det, groups.ora, scene, mode=1)
    assert direct["n_tables"] == 0
    assert direct["n_lds_atomics"] == sum(2 * 64 * -(-min(VOTE_CHUNK, c - k) // 64) * len(al) for k in range(0, c, VOTE_CHUNK))


# ---- (b) table width ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [63, 64, 150])
def test_tables_at_the_width_limit(groups, det, mixed, m):
    """m hits inside one alpha bin, in cells away from its ends: some cell has all m on one side, so the largest count is m --
    63 is the last narrow table, 64 the first wide one, 150 needs more than seven bits."""
    h, a, b = mixed
    centre = (1.5 * 4 * math.pi / groups.A) / math.pi * 180.0  # the middle of the bin Y = 1
    scene = ring_scene(groups, a, b, sector(centre, m, width_deg=12.0))
    al = hits_of(groups, scene, h)
    assert len(al) == m and len(set(np.floor(al * groups.A / (4 * math.pi)).tolist())) == 1
    assert largest_count(al, groups.A) == m
    for acc32 in (None, 1):
        st = run_one(det, groups.ora, scene, acc32=acc32)
        assert st["n_tables"] == 1


def test_a_run_of_narrow_and_wide_tables(groups, det, mixed):
    """Four tables of one run (191 hits each but the last): the device is free to order a run's hits, so the case only needs
    tables on both sides of the limit whichever way the hits are cut -- 382 hits inside one bin (any 191 of them: wide) and 200
    spread over the circle (any table made of those alone: narrow) -- and is there to be compared cell by cell."""
    h, a, b = mixed
    centre = (1.5 * 4 * math.pi / groups.A) / math.pi * 180.0
    alphas = np.concatenate([sector(centre, 382, width_deg=12.0), spread(200)])
    scene = ring_scene(groups, a, b, alphas)
    al = hits_of(groups, scene, h)
    assert len(al) == 582
    assert largest_count(al[:191], groups.A) > NARROW_MAX and largest_count(al[382:573], groups.A) <= NARROW_MAX
    st = run_one(det, groups.ora, scene)
    assert st["n_tables"] == 4


# ---- (c) a group with a guard-band entry ----------------------------------------------------------------------------------
def test_a_group_with_entries_that_vote_one_by_one():
    """A planar model (every frame the identity): the pairs (origin, point on the +y axis) have alpha_m = 0 exactly, which is
    the edge of a count-table cell -- such entries take the all-zero row and vote hit by hit -- and the pairs (origin, point a
    little below the axis) a small positive alpha_m: the same row, the same X, ordinary cells.  All pairs at about the same
    distance share one bucket (equal normals)."""
    rng = np.random.default_rng(7)
    axis = [[0.0500 + 0.0002 * k, 0.0] for k in range(3)]              # alpha_m = atan2(-0, u) = 0
    below = [[0.0500, -0.004], [0.0504, -0.008], [0.0498, -0.012]]      # alpha_m = atan2(-z, y) > 0, within one bin
    model = np.vstack([_plane([[0.0, 0.0]]), _plane(axis), _plane(below), _plane(rng.uniform(-0.1, 0.1, size=(300, 2)))]).astype(np.float32)
    ora = O.OracleDetector(0.05, 0.05).train_model(model, presampled=True)
    info = ora.info()
    A, n = info["num_angles"], info["n_ref"]
    assert n == model.shape[0] and A == 30
    hsh, alp = ora.pairs()
    h = int(hsh[0, 1])
    row0 = [j for j in range(1, n) if int(hsh[0, j]) == h]
    assert set(range(1, 7)) <= set(row0), "the planted pairs do not share a bucket"
    X = np.floor(alp[0, row0].astype(np.float32) * np.float32(A / (4 * math.pi)) + np.float32(0.5 * A)).astype(np.int64)
    am = alp[0, row0]
    same = X == A // 2
    assert np.sum(same & (am == 0.0)) >= 3 and np.sum(same & (am > 0.0)) >= 3, "no group of row 0 mixes cell-edge and ordinary entries"
    assert records_for(int(np.sum((hsh == h) & ~np.eye(n, dtype=bool)))) >= MIN_RECORDS
    # the scene: the origin and 40 points on the circle of radius 0.05 around it, in the plane
    t = np.linspace(0.3, 2.0 * math.pi - 0.3, 40)
    scene = np.vstack([_plane([[0.0, 0.0]]), _plane(np.stack([0.05 * np.cos(t), 0.05 * np.sin(t)], axis=1))]).astype(np.float32)
    det = PPF3DDetector(0.05, 0.05).trainModel(model, presampled=True)
    assert det.info()["n_tiles"] == 1
    want = ora.accumulator(scene, 0)
    assert int(want.sum(dtype=np.uint64)) >= 40 * 64
    for mode in (0, 1):
        st = check(Workspace(), det, ora, scene, 1.0 / scene.shape[0], [0], {0: want}, vote_mode=mode)
        assert st["n_retries"] == 0 and st["n_acc32_items"] == 0
        assert (st["n_tables"] >= 1) == (mode == 0)


# ---- (d) tilings and cells, (e) chunking -----------------------------------------------------------------------------------
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


def ring_bucket_entries(c):
    """Entries of the bucket of the case's ring (955 hits around scene row 1000: five count tables), per tile."""
    hsh = c.ora.pairs()[0]
    n = c.N
    first = c.scene[c.ring_rows[0]]
    _, _, h = O.pair_feature(c.scene[c.ring_ref, :3], c.scene[c.ring_ref, 3:], first[:3], first[3:], c.ora.info()["angle_step"],
                             c.ora.info()["distance_step"])
    rows_of = np.nonzero((hsh == h) & ~np.eye(n, dtype=bool))[0]
    return [int(np.sum(rows_of // c.T == t)) for t in range(c.n_tiles)]


@pytest.mark.parametrize("acc32", [None, 1, 2])
@pytest.mark.parametrize("tiling", TILINGS)
def test_tilings_and_cell_widths(cases, tiling, acc32):
    """One tile, three tiles and ten tiles of odd height; 16-bit cells, 32-bit cells for everything (PPF_OPT_ACC32 = 1) and for
    the flagged items only (2)."""
    c = cases(tiling)
    per_tile = ring_bucket_entries(c)
    assert max(records_for(e) for e in per_tile) >= MIN_RECORDS
    ws = Workspace()
    if acc32 is not None:
        ws.set_option(_capi.PPF_OPT_ACC32, acc32)
    st = c.run(ws, 0)
    assert st["n_retries"] == 0 and st["n_tables"] > 0 and st["n_lds_atomics"] < st["n_votes"]
    assert st["n_acc32_items"] == (len(c.refs) * c.n_tiles if acc32 == 1 else 0)


@pytest.mark.parametrize("num_angles", [20, 40])
def test_other_alpha_resolutions(cases, num_angles):
    """20 bins: count tables and group records with another X range; 40 (> 31): direct votes, nothing of this applies."""
    c = cases(0, num_angles)
    st = c.run(Workspace(), 0)
    assert st["n_retries"] == 0 and st["n_acc32_items"] == 0
    assert (st["n_tables"] > 0) == (num_angles <= 31)


def test_s2b_with_an_edge_cloud(cases):
    c = cases(0)
    keep = np.arange(c.scene.shape[0]) % 5 == 1
    keep[[part for _, part, _ in c.planted]] = True
    keep[c.ring_rows] = True
    edge = np.ascontiguousarray(c.scene[keep])
    st = check(Workspace(), c.det, c.ora, c.scene, 1.0, c.refs, {}, ref_stride=REF_STRIDE, vote_mode=0, edge=edge)
    assert st["n_paired"] == edge.shape[0] and st["n_retries"] == 0 and st["n_acc32_items"] == 0 and st["n_tables"] > 0


def test_a_16_bit_overflow_is_voted_again():
    """The spot of test_gpu_accumulators (1,000 scene points in one spot seen from the reference point, 200 model points in one
    spot seen from a model point: about 200,000 votes in one cell).  The 200 entries of the origin's row share their X: one
    group, fifty group records.  Cold workspace: the 16-bit item is flagged by the votes it finds and voted again with 32-bit
    cells; warm: 32-bit cells from the start."""
    rng = np.random.default_rng(3)
    model, H = _around_the_half_boundary(np.vstack([_far(rng, 200), _plane(rng.uniform(-0.1, 0.1, size=(40, 2)))]))
    scene = np.vstack([ORIGIN, _lifted_partner()[None, :], _far(rng, 1000), _plane(rng.uniform(-0.1, 0.1, size=(40, 2)))]).astype(np.float32)
    det = PPF3DDetector(0.05, 0.05).trainModel(model, presampled=True)
    ora = O.OracleDetector(0.05, 0.05).train_model(model, presampled=True)
    hsh, alp = ora.pairs()
    A, n = ora.info()["num_angles"], ora.info()["n_ref"]
    far = [j for j in range(n) if j != H - 1 and abs(float(model[j, 1]) - 0.1) < 1e-3 and abs(float(model[j, 2]) - 0.02) < 1e-3]
    assert len(far) == 200 and len({int(hsh[H - 1, j]) for j in far}) == 1
    X = np.floor(alp[H - 1, far].astype(np.float32) * np.float32(A / (4 * math.pi)) + np.float32(0.5 * A))
    assert len(set(X.tolist())) == 1, "the spot's entries of the origin's row are more than one group"
    assert records_for(int(np.sum((hsh == hsh[H - 1, far[0]]) & ~np.eye(n, dtype=bool)))) >= MIN_RECORDS
    assert S.Recount(ora).spills(scene, 0, 1, H - 1) >= 1
    want = {0: ora.accumulator(scene, 0)}
    assert want[0].max() > 65535
    ws = Workspace()
    for _ in range(2):
        st = check(ws, det, ora, scene, 1.0 / scene.shape[0], [0], want, vote_mode=0)
        assert st["n_retries"] == 0 and st["n_acc32_items"] == 1 and st["n_tables"] >= 1
