"""k_vote stages one record per WORK ITEM and cuts a reference point's segments by items: a segment takes items until the
staging area is full and may start and end inside a run.  The scenes here give one reference point (scene row 0) runs of
chosen sizes on buckets of chosen sizes, built like those of test_gpu_sparse_tables: a model pair (a, b), the scene = a plus
copies of b turned about a's normal, so that every copy is a hit in the bucket of (a, b).  Every scene is first confirmed with
the CPU oracle alone (which buckets are hit how often, how many entries they hold, and from that the items of the reference
point, by the formulas of the staging code); then the device's accumulator is compared with the oracle's cell by cell -- in
count-table mode and with direct votes, with the default staging area and with PPF_OPT_RUN_STAGING = 64, with 16- and 32-bit
cells -- and n_votes, n_lds_atomics and the vote triple must not depend on the size of the staging area.

What the item counts rest on (yolo_ppf_pose_estimation_amd/csrc/ppf_match_kernels.h, ppf_train_kernels.h):
  records of a bucket of n entries in a model of one tile      32 * ((n - 1) // 64) + min((n - 1) % 64, 31) + 1
  items of a run of m hits on c records   count tables (m >= 24, c >= 32, count-table mode)   ceil(m / 191) * ceil(c / 1024)
                                          direct                                              ceil(m / 24) * ceil(c / 1024)
  item records the staging area holds     ((runs + 1) * 24 + 15) // 16 for a size of `runs`: 64 -> 98; the default is what
                                          the LDS leaves next to the accumulator tile, 704 .. 1,024 in steps of 64
  order of a reference point's runs       many-hit runs (m >= 24, count-table mode) by ascending hash slot, then the others
"""
import math

import numpy as np
import pytest

import oracle_lib as O
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
from yolo_ppf_pose_estimation_amd.device import Workspace

pytestmark = pytest.mark.gpu

DISTANCE = 0.05
SMALL, C2_STEP = 0.08, 0.036     # the bottle at 430 rows; at 2,000 rows (C2's model: buckets of up to 20 chunks of records)
MIN_HITS, SUB, CHUNK = 24, 191, 1024
DEG = math.pi / 180.0
LDS_BYTES, LDS_FIXED_LEAST, RUN_SEG, RUN_SEG_MAX = 160 * 1024, 256 + 16928 + 16 * 1312, 704, 1024


def item_seg(run_seg):
    return ((run_seg + 1) * 24 + 15) // 16


def default_item_seg(tile_refs, num_angles):
    acc_words = 64 + 2 * ((num_angles + 1) | 1) + ((tile_refs + 1) // 2) * num_angles + 1
    more = (LDS_BYTES - LDS_FIXED_LEAST - 4 * acc_words) // (64 * 24)
    return item_seg(min(RUN_SEG_MAX, RUN_SEG + 64 * max(more, 0)))


def records(n):
    return 32 * ((n - 1) // 64) + min((n - 1) % 64, 31) + 1 if n else 0


def items_of(m, n, mode):
    c = records(n)
    if mode == 0 and m >= MIN_HITS and c >= 32:
        return -(-m // SUB) * -(-c // CHUNK)
    return -(-m // MIN_HITS) * -(-c // CHUNK)


def _rot(axis, t):
    k = np.asarray(axis, dtype=np.float64)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


class Rings:
    """A model, its oracle and its device twin, and scene points for the reference point a = model point `a`: every model pair
    (i, j), moved rigidly so that i lands on a (position and normal), gives a point that has with a the features of (i, j) --
    so every bucket of the model can be hit from a, one point per bucket here, the buckets of most entries first."""

    def __init__(self, bottle, sampling, a, limit):
        self.ora = O.OracleDetector(sampling, DISTANCE).train_model(bottle)
        self.info = self.ora.info()
        self.A, self.slots = self.info["num_angles"], self.info["slots"]
        self.model = self.ora.sampled_model().astype(np.float64)
        n = self.info["n_ref"]
        hsh, _ = self.ora.pairs()
        self.slot = hsh.astype(np.int64) % self.slots
        self.slot[np.eye(n, dtype=bool)] = -1
        u, first, c = np.unique(self.slot.ravel(), return_index=True, return_counts=True)
        keep = u >= 0
        self.size = dict(zip(u[keep].tolist(), c[keep].tolist()))
        self.first_pair = dict(zip(u[keep].tolist(), first[keep].tolist()))
        self.a = a
        self.det = PPF3DDetector(sampling, DISTANCE).trainModel(bottle)
        di = self.det.info()
        assert (di["n_ref"], di["n_tiles"]) == (n, 1), "the item counts below are those of a model of one tile"
        self.cap = {0: default_item_seg(di["tile_refs"], self.A), 64: item_seg(64)}
        self.partners = self._partners(limit)
        self._want = {}

    def feature(self, p1, n1, p2, n2):
        return O.pair_feature(p1, n1, p2, n2, self.info["angle_step"], self.info["distance_step"])

    def _moved(self, i, j):
        """Model point j as seen from i, carried over to a."""
        pa, na = self.model[self.a, :3], self.model[self.a, 3:] / np.linalg.norm(self.model[self.a, 3:])
        ni = self.model[i, 3:] / np.linalg.norm(self.model[i, 3:])
        ax, c = np.cross(ni, na), float(np.dot(ni, na))
        if np.linalg.norm(ax) < 1e-9:
            if c < 0:
                return None
            R = np.eye(3)
        else:
            R = _rot(ax / np.linalg.norm(ax), math.atan2(np.linalg.norm(ax), c))
        return np.concatenate([pa + R @ (self.model[j, :3] - self.model[i, :3]), R @ self.model[j, 3:]])

    def _partners(self, limit, margin=0.1):
        """[(point, slot, entries)], one point per bucket: all four features of (a, point) away from their bin edges (the
        turned copies are rounded to fp32 and must stay in the bucket), the point off a's normal axis."""
        out = []
        steps = np.array([self.info["angle_step"]] * 3 + [self.info["distance_step"]])
        pa, na = self.model[self.a, :3], self.model[self.a, 3:]
        n = self.model.shape[0]
        for s in sorted(self.size, key=lambda s: -self.size[s]):
            pt = self._moved(*divmod(self.first_pair[s], n))
            if pt is None:
                continue
            pt32 = pt.astype(np.float32)
            f, _, h = self.feature(pa, na, pt32[:3], pt32[3:])
            frac = np.mod(f / steps, 1.0)
            d = pt[:3] - pa
            if h % self.slots != s or frac.min() < margin or frac.max() > 1.0 - margin:
                continue
            if np.linalg.norm(np.cross(d, na)) < 0.2 * np.linalg.norm(d) * np.linalg.norm(na):
                continue
            out.append((pt, s, self.size[s]))
            if len(out) == limit:
                break
        return out

    def ring(self, k, m):
        """m copies of partner k turned about a's normal, alpha_s spread over the circle."""
        pa, na = self.model[self.a, :3], self.model[self.a, 3:]
        pt = self.partners[k][0]
        ax = na / np.linalg.norm(na)
        return np.array([np.concatenate([pa + _rot(ax, t) @ (pt[:3] - pa), _rot(ax, t) @ pt[3:]])
                         for t in (np.linspace(-179.0, 179.0, m) if m > 1 else np.array([40.0])) * DEG])

    def scene(self, parts):
        """Row 0 = model point a, then a ring of m copies of partner k for every (k, m) of `parts`; confirmed by the oracle:
        reference point 0 has exactly these runs.  Returns (scene, [(slot, m, entries)] in the order of `parts`)."""
        sc = np.vstack([self.model[self.a][None, :]] + [self.ring(k, m) for k, m in parts]).astype(np.float32)
        got = {}
        for k in range(1, sc.shape[0]):
            _, _, h = self.feature(sc[0, :3], sc[0, 3:], sc[k, :3], sc[k, 3:])
            if h % self.slots in self.size:
                got[h % self.slots] = got.get(h % self.slots, 0) + 1
        runs = [(self.partners[k][1], m, self.partners[k][2]) for k, m in parts]
        assert got == {s: m for s, m, _ in runs}, "the scene does not give the intended runs"
        return sc, runs

    def want(self, key, scene):
        if key not in self._want:
            acc = self.ora.accumulator(scene, 0)
            one = self.ora.match(scene, relative_scene_sample_step=1.0, presampled=True, cluster=False, ref_list=[0])
            assert int(acc.sum(dtype=np.uint64)) == int(one["votes_per_ref"][0])
            self._want[key] = (acc, one["triples"][0].copy(), int(one["votes_per_ref"][0]))
        return self._want[key]


def total_items(runs, mode):
    return sum(items_of(m, n, mode) for _, m, n in runs)


def device(rg, scene, mode, staging, acc32=0):
    """(accumulator of reference point 0, vote triple, statistics) of one call on a fresh workspace."""
    ws = Workspace()
    if staging:
        ws.set_option(_capi.PPF_OPT_RUN_STAGING, staging)
    if acc32:
        ws.set_option(_capi.PPF_OPT_ACC32, 1)
    n = scene.shape[0]
    acc = ws.accumulators(rg.det, scene, 1.0, ref_offset=0, ref_stride=n, vote_mode=mode)
    res = ws.results(n)
    assert acc.shape[0] == res["n_ref"] == 1
    return acc[0], res["triples"][0], ws.stats()


def check(rg, key, scene, mode, acc32s=(0, 1)):
    """Cell by cell against the oracle with the default staging area and with the smallest, 16- and 32-bit cells; the
    statistics may not depend on the staging.  Returns the statistics of the 16-bit run with default staging.

    n_lds_atomics is a function of the items alone wherever the column masks of the count tables are: with direct votes
    always; in count-table mode when no choice of the device can change a mask -- the device is free in which 191 hits of a
    longer run share a table, and a table's mask is the set of its hits' Y values.  Every scene of this function has only
    one-table runs or (the 192-hit run, asserted where it is built) runs whose every Y value has at least two hits, so that
    any 191 of them set all columns and the one left over sets two."""
    want, triple, votes = rg.want(key, scene)
    first = None
    for acc32 in acc32s:
        seen = []
        for staging in (0, 64):
            acc, tr, st = device(rg, scene, mode, staging, acc32)
            np.testing.assert_array_equal(acc, want, err_msg=f"mode {mode}, staging {staging}, acc32 {acc32}")
            np.testing.assert_array_equal(tr, triple)
            assert st["n_votes"] == votes and st["n_retries"] == 0
            seen.append(st)
        assert seen[0]["n_lds_atomics"] == seen[1]["n_lds_atomics"] and seen[0]["n_votes"] == seen[1]["n_votes"]
        assert seen[0]["n_tables"] == seen[1]["n_tables"]
        first = first or seen[0]
    return first


@pytest.fixture(scope="module")
def small(bottle):
    return Rings(bottle, SMALL, a=5, limit=10 ** 6)


@pytest.fixture(scope="module")
def big(bottle):
    return Rings(bottle, C2_STEP, a=5, limit=2800)


def fill(rg, cands, target, hits, mode):
    """[(partner, hits)] out of the partners `cands` (indices) whose items add up to `target` exactly: greedily the buckets of
    most items first, one run per bucket."""
    parts, left = [], target
    for k in sorted(cands, key=lambda k: -items_of(hits, rg.partners[k][2], mode)):
        it = items_of(hits, rg.partners[k][2], mode)
        if it <= left:
            parts.append((k, hits))
            left -= it
        if left == 0:
            return parts
    raise AssertionError(f"the model's buckets do not add up to {target} items")


# ---- 1. item count at the staging capacity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("staging", [64, 0])
@pytest.mark.parametrize("delta", ["cap-1", "cap", "cap+1", "2cap+1"])
def test_item_count_at_the_staging_capacity(big, delta, staging, mode):
    """One-hit runs, each on another bucket: a run has as many items as its bucket has chunks of 1,024 records (1 .. 20 on this
    model) in both voting modes, so a few hundred scene points give the 1,346 items of the default area (98 of the smallest)
    and one less, one more and twice as many + 1: a segment that is full to the last record, one with one record left, a
    second segment of one item, a third."""
    cap = big.cap[staging]
    assert cap == (98 if staging else 1346)
    target = {"cap-1": cap - 1, "cap": cap, "cap+1": cap + 1, "2cap+1": 2 * cap + 1}[delta]
    scene, runs = big.scene(fill(big, range(len(big.partners)), target, 1, mode))
    assert total_items(runs, 0) == total_items(runs, 1) == target and scene.shape[0] <= 3000
    check(big, ("cap", delta, staging), scene, mode)


# ---- 2. a count-table run of several items across a segment boundary ---------------------------------------------------------
def _heavy_scene(rg, staging, ahead):
    """A run R of 192 hits (two count tables) on a bucket of more than 1,024 records, behind many-hit runs (24 hits each, on
    buckets of smaller slots: they come first in the run list) whose items add up to capacity - ahead."""
    P = rg.partners
    R = max((k for k in range(len(P)) if records(P[k][2]) > CHUNK), key=lambda k: P[k][1])
    ni = items_of(192, P[R][2], 0)
    assert ni >= 4
    before = [k for k in range(len(P)) if P[k][1] < P[R][1] and P[k][2] >= 64]
    parts = fill(rg, before, rg.cap[staging] - ahead, MIN_HITS, 0) + [(R, 192)]
    scene, runs = rg.scene(parts)
    assert all(s < runs[-1][0] and items_of(m, n, 0) >= 1 and m >= MIN_HITS for s, m, n in runs[:-1])
    assert total_items(runs[:-1], 0) == rg.cap[staging] - ahead and scene.shape[0] <= 4000
    ys = [int(math.floor(O.alpha(scene[0, :3], scene[0, 3:], scene[k, :3]) * rg.A / (4 * math.pi))) + 8 for k in range(scene.shape[0] - 192, scene.shape[0])]
    assert set(ys) == set(range(16)) and min(ys.count(y) for y in range(16)) >= 2  # R's tables have the same masks whichever hit is left over
    return scene, ni


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ahead", [0, 1, -1])
def test_a_count_table_run_of_several_items_across_a_segment_boundary(big, ahead, mode):
    """`ahead` = records of the smallest staging area (98) left when R's turn comes: 0: R starts the second segment; 1: the cut
    falls behind R's first item; -1 (counted from R's end): the cut falls in front of R's last item.  Aimed at the smallest
    area only.  Many-hit runs come first in the run list, so only many-hit runs can stand in front of R, at 24 scene points
    for a run of one table; this model's buckets of more than one chunk give 195 items for 1,700 points (51 of two chunks, 10 of
    three, 8 of four, one each of six, eight and seventeen), the other 1,150 items in front of the default area's 1,346th would
    take 27,600 points of one-item runs.  (At the default size runs are cut in the 2 x capacity + 1 scene of case 1: direct
    runs of several chunks.)  Every scene is run with both sizes all the same.  (Direct votes make other items of the same scene: more of them, cut elsewhere.)"""
    if ahead < 0:
        _, ni = _heavy_scene(big, 64, 1)
        ahead = ni - 1
    scene, ni = _heavy_scene(big, 64, ahead)
    assert 0 <= ahead < ni
    st = check(big, ("heavy", ahead), scene, mode)
    assert st["n_tables"] >= 2 if mode == 0 else st["n_tables"] == 0


# ---- 3. a direct run longer than a whole segment -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hits", [24, 25, 49, 98 * 24 + 1])
def test_a_direct_run_on_a_tiny_bucket(small, hits, mode):
    """A bucket of fewer than 32 records never gets a count table: a run of m hits on it is ceil(m / 24) direct items in both
    modes -- 1, 2, 3, and one more than the smallest staging area holds (the run starts and ends two segments and fills one)."""
    tiny = [k for k in range(len(small.partners)) if records(small.partners[k][2]) < 32]
    assert tiny
    scene, runs = small.scene([(tiny[0], hits)])
    assert total_items(runs, 0) == total_items(runs, 1) == -(-hits // MIN_HITS) and scene.shape[0] <= 3000
    st = check(small, ("tiny", hits), scene, mode)
    # (k_group hands a run of 24 hits its count tables before any tile's records are known; k_vote leaves them alone here)
    assert st["n_tables"] == (0 if mode else -(-hits // SUB)) and st["n_lds_atomics"] >= st["n_votes"], "the run did not vote directly"


# ---- 4. a 16-bit cell that overflows; a model of two tiles -------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_a_run_longer_than_a_segment_whose_cell_overflows(mode):
    """The spot of test_gpu_accumulators (1,000 scene points in one spot seen from the reference point, 200 model points in the
    same spot seen from a model point: one run of about 1,000 hits on a bucket of about 40,000 entries, 200,000 votes in one
    cell): the 16-bit launch flags it, the listed 32-bit launch votes it again, each with a run of more items than the smallest
    staging area holds."""
    import test_gpu_accumulators as T
    rng = np.random.default_rng(3)
    model, H = T._around_the_half_boundary(np.vstack([T._far(rng, 200), T._plane(rng.uniform(-0.1, 0.1, size=(40, 2)))]))
    scene = np.vstack([T.ORIGIN, T._lifted_partner()[None, :], T._far(rng, 1000), T._plane(rng.uniform(-0.1, 0.1, size=(40, 2)))]).astype(np.float32)
    det = PPF3DDetector(0.05, 0.05).trainModel(model, presampled=True)
    ora = O.OracleDetector(0.05, 0.05).train_model(model, presampled=True)
    want = ora.accumulator(scene, 0)
    assert want.max() > 65535
    hsh, _ = ora.pairs()
    slot = hsh.astype(np.int64) % ora.info()["slots"]
    biggest = int(np.unique(slot[~np.eye(model.shape[0], dtype=bool)], return_counts=True)[1].max())
    assert items_of(900, biggest, mode) > item_seg(64)  # the spot's run (nearly all of the 1,000 points hit its bucket): 5 tables or 38 hit ranges x 20 chunks
    seen = []
    for staging in (0, 64):
        ws = Workspace()
        if staging:
            ws.set_option(_capi.PPF_OPT_RUN_STAGING, staging)
        acc = ws.accumulators(det, scene, 1.0 / scene.shape[0], vote_mode=mode)
        st = ws.stats()
        np.testing.assert_array_equal(acc[0], want)
        assert st["n_acc32_items"] == 1 and st["n_retries"] == 0 and st["n_votes"] == int(want.sum(dtype=np.uint64))
        seen.append(st)
    # count-table mode: the spot's 1,000 hits have alpha_s within a fraction of a degree of each other, across a Y boundary or
    # not as the dice fell; which 191 of them share a table is the device's choice, varies from call to call, and with it the
    # tables' column masks and the counted atomics (see check()).  Direct votes: a function of the items alone.
    if mode == 1:
        assert seen[0]["n_lds_atomics"] == seen[1]["n_lds_atomics"]


@pytest.mark.parametrize("mode", [0, 1])
def test_a_model_of_two_tiles(bottle, mode):
    """More than 2,085 rows: two tiles, every bucket's records split between them, so a tile's items are not those of the
    formulas above; the scene is one of the capacity scenes' kind (one-hit runs on the buckets of most entries) with as many
    items over both tiles as two default staging areas hold, or more."""
    step = 0.0345
    ora = O.OracleDetector(step, DISTANCE).train_model(bottle)
    det = PPF3DDetector(step, DISTANCE).trainModel(bottle)
    info = det.info()
    assert info["n_ref"] == ora.info()["n_ref"] > 2085 and info["n_tiles"] == 2
    model = ora.sampled_model().astype(np.float64)
    a = 5
    hsh, _ = ora.pairs()
    slot = hsh.astype(np.int64) % ora.info()["slots"]
    u, c = np.unique(slot[~np.eye(model.shape[0], dtype=bool)], return_counts=True)
    size = dict(zip(u.tolist(), c.tolist()))
    order = sorted(range(model.shape[0]), key=lambda b: -size.get(int(slot[a, b]), 0) if b != a else 1)
    scene = np.vstack([model[a][None, :]] + [model[b][None, :] for b in order[:2000]]).astype(np.float32)
    n_items = 0
    for k in range(1, scene.shape[0]):
        _, _, h = O.pair_feature(scene[0, :3], scene[0, 3:], scene[k, :3], scene[k, 3:], ora.info()["angle_step"], ora.info()["distance_step"])
        n_items += -(-records(size.get(h % ora.info()["slots"], 0)) // CHUNK)
    assert n_items >= 2 * default_item_seg(info["tile_refs"], info["num_angles"])
    want = ora.accumulator(scene, 0)
    seen = []
    for staging in (0, 64):
        ws = Workspace()
        if staging:
            ws.set_option(_capi.PPF_OPT_RUN_STAGING, staging)
        acc = ws.accumulators(det, scene, 1.0, ref_offset=0, ref_stride=scene.shape[0], vote_mode=mode)
        st = ws.stats()
        np.testing.assert_array_equal(acc[0], want)
        assert st["n_votes"] == int(want.sum(dtype=np.uint64)) and st["n_retries"] == 0
        seen.append(st)
    assert seen[0]["n_lds_atomics"] == seen[1]["n_lds_atomics"]
