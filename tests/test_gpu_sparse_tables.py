"""Count tables with few non-zero columns: k_vote casts the counted atomics of a table's set columns only (the column mask
k_tables derives from the Y values of the table's hits).  The scenes here give one reference point a run of a chosen size in
chosen Y columns: a model pair (a, b) of a big bucket, the scene = a plus m copies of b turned about a's normal, so that all
m pairs keep a's features (one bucket) while alpha_s follows the angle of the turn.  Every scene is first confirmed with the
CPU oracle alone (run size, Y values); then the device's accumulators are compared with the oracle's cell by cell, in both
voting modes and with 32-bit cells, and the statistics are checked."""
import math

import numpy as np
import pytest
import torch

import oracle_lib as O
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
from yolo_ppf_pose_estimation_amd.device import Workspace

pytestmark = pytest.mark.gpu

SAMPLING, DISTANCE = 0.08, 0.05  # the bottle at 430 rows
MIN_HITS = 24                    # PPF_AGG_MIN_HITS: runs with at least this many hits vote through count tables
DEG = math.pi / 180.0


def _rot(axis, t):
    """Rotation matrix of angle t about the unit vector axis (Rodrigues)."""
    k = np.asarray(axis, dtype=np.float64)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


class Rings:
    """The small model, its oracle, and the model pairs (a, b) that scenes are built from."""

    def __init__(self, bottle):
        self.ora = O.OracleDetector(SAMPLING, DISTANCE).train_model(bottle)
        self.info = self.ora.info()
        self.A = self.info["num_angles"]
        self.model = self.ora.sampled_model().astype(np.float64)
        n = self.info["n_ref"]
        hsh, _ = self.ora.pairs()
        self.hsh = hsh
        off = ~np.eye(n, dtype=bool)
        u, c = np.unique(hsh[off], return_counts=True)
        self.bucket_size = dict(zip(u.tolist(), c.tolist()))

    def feature(self, p1, n1, p2, n2):
        return O.pair_feature(p1, n1, p2, n2, self.info["angle_step"], self.info["distance_step"])

    def partners(self, a, lo=64, hi=1500, count=1, margin=0.25):
        """Model points b whose pair (a, b) lies in a bucket of lo..hi entries with all four features away from their bin
        edges (the turned copies are rounded to fp32: they must stay in the bucket); one b per bucket."""
        out, seen = [], set()
        steps = np.array([self.info["angle_step"]] * 3 + [self.info["distance_step"]])
        for b in range(self.model.shape[0]):
            if b == a:
                continue
            h = int(self.hsh[a, b])
            if h in seen or not lo <= self.bucket_size.get(h, 0) <= hi:
                continue
            f, _, h2 = self.feature(self.model[a, :3], self.model[a, 3:], self.model[b, :3], self.model[b, 3:])
            frac = np.mod(f / steps, 1.0)
            if h2 != h or frac.min() < margin or frac.max() > 1.0 - margin:
                continue
            # b off a's normal axis, or turning it moves nothing
            d = self.model[b, :3] - self.model[a, :3]
            if np.linalg.norm(np.cross(d, self.model[a, 3:])) < 0.2 * np.linalg.norm(d):
                continue
            seen.add(h)
            out.append(b)
            if len(out) == count:
                break
        assert len(out) == count, "the model has too few usable pairs for this reference point"
        return out

    def ring(self, a, b, alphas):
        """Copies of b turned about a's normal so that alpha_s of (a, copy) is each of `alphas` (radians, in (-pi, pi))."""
        pa, na = self.model[a, :3], self.model[a, 3:]
        pb, nb = self.model[b, :3], self.model[b, 3:]

        def turned(t):
            R = _rot(na / np.linalg.norm(na), t)
            return np.concatenate([pa + R @ (pb - pa), R @ nb])

        a0 = O.alpha(pa, na, turned(0.0)[:3])
        a1 = O.alpha(pa, na, turned(0.01)[:3])
        sign = 1.0 if math.remainder(a1 - a0, 2 * math.pi) > 0 else -1.0
        return np.array([turned(sign * (al - a0)) for al in alphas])

    def scene(self, a, rings):
        """Row 0 = model point a, then the rings' points."""
        return np.vstack([self.model[a][None, :]] + list(rings)).astype(np.float32)

    def runs_of(self, scene, i=0):
        """By the oracle alone: {bucket hash: Y + 8 of its hits, in scene order} of the scene's reference point i, model buckets only."""
        runs = {}
        for k in range(scene.shape[0]):
            if k == i:
                continue
            _, _, h = self.feature(scene[i, :3], scene[i, 3:], scene[k, :3], scene[k, 3:])
            if h in self.bucket_size:
                al = O.alpha(scene[i, :3], scene[i, 3:], scene[k, :3])
                runs.setdefault(h, []).append(int(math.floor(al * self.A / (4 * math.pi))) + 8)
        return runs


@pytest.fixture(scope="module")
def rings(bottle):
    return Rings(bottle)


@pytest.fixture(scope="module")
def det(bottle):
    return PPF3DDetector(SAMPLING, DISTANCE).trainModel(bottle)


def sector(centre_deg, m, width_deg=20.0):
    return (centre_deg + np.linspace(-0.5, 0.5, m) * width_deg) * DEG


def straddle(m, width_deg=20.0):
    """A sector across alpha_s = +-pi: half of the hits just below +pi, half just above -pi."""
    h = m // 2
    return np.concatenate([(180.0 - np.linspace(0.5, 0.5 * width_deg, h)) * DEG,
                           (-180.0 + np.linspace(0.5, 0.5 * width_deg, m - h)) * DEG])


def spread(m):
    return np.linspace(-179.0, 179.0, m) * DEG


def columns(ys):
    """The 17-bit column mask of hits with these Y + 8."""
    occ = 0
    for y in ys:
        occ |= 1 << y
    return (occ | (occ << 1)) & 0x1FFFF


def check_scene(rings, det, scene, refs=(0,)):
    """Device accumulators of the reference points `refs` (auto and direct voting, 16- and 32-bit cells) against the
    oracle's, cell by cell, and the triples of every reference point; returns the statistics of an automatic run over those reference points."""
    n = scene.shape[0]
    want_all = rings.ora.match(scene, relative_scene_sample_step=1.0, presampled=True, cluster=False)
    want_acc = {}
    for r in refs:
        want = want_acc[r] = rings.ora.accumulator(scene, r)
        a0 = det.accumulators(scene, 1.0, ref_offset=r, ref_stride=n, vote_mode=0)
        a1 = det.accumulators(scene, 1.0, ref_offset=r, ref_stride=n, vote_mode=1)
        assert a0.shape[0] == 1
        np.testing.assert_array_equal(a0[0], want)
        np.testing.assert_array_equal(a1[0], a0[0])
    for mode in (0, 1):
        got = det.raw_votes(scene, 1.0, 0.05, presampled=True, vote_mode=mode)
        np.testing.assert_array_equal(got["triples"], want_all["triples"])
        assert got["stats"]["n_votes"] == int(want_all["votes_per_ref"].sum())
    for mode in (0, 1):  # 32-bit cells: the other instantiation of the same masked loop
        ws = Workspace()
        ws.set_option(_capi.PPF_OPT_ACC32, 1)
        d = torch.from_numpy(scene).cuda()
        ws.match_device(det, d.data_ptr(), n, 6, 1.0, 0.05, presampled=True, skip_clustering=True, vote_mode=mode)
        res = ws.results(n)
        np.testing.assert_array_equal(res["triples"], want_all["triples"])
        assert res["stats"]["n_votes"] == int(want_all["votes_per_ref"].sum())
        for r in refs:  # and cell by cell, on the same workspace
            a32 = ws.accumulators(det, scene, 1.0, ref_offset=r, ref_stride=n, vote_mode=mode)
            assert a32.shape[0] == 1 and ws.stats()["n_acc32_items"] == det.info()["n_tiles"]
            np.testing.assert_array_equal(a32[0], want_acc[r])
    one = det.raw_votes(scene, 1.0, 0.05, presampled=True, ref_offset=refs[0], ref_stride=n, vote_mode=0)
    assert one["n_ref"] == 1
    np.testing.assert_array_equal(one["triples"][0], want_all["triples"][refs[0]])
    assert one["stats"]["n_votes"] == int(want_all["votes_per_ref"][refs[0]])
    return one["stats"]


def one_run(rings, a, b, alphas):
    """Scene of one ring, confirmed by the oracle: reference point 0 has exactly one run, of len(alphas) hits."""
    scene = rings.scene(a, [rings.ring(a, b, alphas)])
    runs = rings.runs_of(scene)
    h = int(rings.hsh[a, b])
    assert list(runs) == [h] and len(runs[h]) == len(alphas), "the scene does not give the intended run"
    return scene, runs[h]


A_REF = 5  # the model point scenes are built around


@pytest.mark.parametrize("m", [24, 64, 191])
def test_a_sector_of_20_degrees_sets_two_or_three_columns(rings, det, m):
    b = rings.partners(A_REF)[0]
    scene, ys = one_run(rings, A_REF, b, sector(40.0, m))
    assert len(set(ys)) <= 2 and bin(columns(ys)).count("1") <= 3
    sparse = check_scene(rings, det, scene)
    scene_d, ys_d = one_run(rings, A_REF, b, spread(m))
    assert columns(ys_d) == 0x1FFFF
    dense = check_scene(rings, det, scene_d)
    assert sparse["n_tables"] == dense["n_tables"] == 1
    assert sparse["n_lds_atomics"] < dense["n_lds_atomics"], "the all-zero columns of the sector's table were cast"


def test_a_sector_across_plus_minus_pi_sets_columns_0_and_16(rings, det):
    b = rings.partners(A_REF)[0]
    scene, ys = one_run(rings, A_REF, b, straddle(64))
    assert set(ys) == {0, 15} and columns(ys) == 0b11000000000000011
    sparse = check_scene(rings, det, scene)
    dense = check_scene(rings, det, one_run(rings, A_REF, b, spread(64))[0])
    assert sparse["n_lds_atomics"] < dense["n_lds_atomics"]


@pytest.mark.parametrize("m", [192, 400])
def test_several_tables_of_one_run(rings, det, m):
    """More than 191 hits: two or three tables of one run; the first 191 angles in one sector, the next 191 opposite, the
    rest in a third.  By the oracle the run's hits, taken 191 at a time in scene order, have pairwise different column masks
    (the device is free to order a run's hits otherwise: whatever tables it forms, the accumulators are the oracle's)."""
    b = rings.partners(A_REF)[0]
    rest = [sector(80.0, min(m - 191, 191))] if m - 191 > 1 else [np.array([80.0 * DEG])]
    if m > 382:
        rest.append(sector(0.0, m - 382))
    scene, ys = one_run(rings, A_REF, b, np.concatenate([sector(-100.0, 191)] + rest))
    masks = [columns(ys[k:k + 191]) for k in range(0, m, 191)]
    assert len(masks) == (m + 190) // 191 == len(set(masks)) and 0x1FFFF not in masks
    st = check_scene(rings, det, scene)
    assert st["n_tables"] == (m + 190) // 191


def test_many_tables_with_different_masks_on_one_reference_point(rings, det):
    """More count-table items than k_vote has waves, each table in another sector (a few over the whole circle): a wave that
    takes a second item meets another mask than its first; a stale mask would skip columns that count."""
    n_runs = 24
    bs = rings.partners(A_REF, count=n_runs, margin=0.2)
    parts = []
    for k, b in enumerate(bs):
        parts.append(rings.ring(A_REF, b, spread(48) if k % 6 == 5 else sector(-165.0 + 41.0 * (k % 9), MIN_HITS + k % 5)))
    scene = rings.scene(A_REF, parts)
    runs = rings.runs_of(scene)
    big = [v for v in runs.values() if len(v) >= MIN_HITS]
    assert len(big) >= n_runs and len({columns(v) for v in big}) >= 8
    st = check_scene(rings, det, scene)
    assert st["n_tables"] >= n_runs > 16


def test_two_reference_points_with_rings_in_different_sectors(rings, det):
    a2 = 200
    b1, b2 = rings.partners(A_REF)[0], rings.partners(a2)[0]
    r1, r2 = rings.ring(A_REF, b1, sector(120.0, 64)), rings.ring(a2, b2, sector(-60.0, 48))
    scene = np.vstack([rings.model[A_REF][None, :], r1, rings.model[a2][None, :], r2]).astype(np.float32)
    i2 = 1 + r1.shape[0]
    h1, h2 = int(rings.hsh[A_REF, b1]), int(rings.hsh[a2, b2])
    ys1, ys2 = rings.runs_of(scene, 0).get(h1, []), rings.runs_of(scene, i2).get(h2, [])
    assert len(ys1) >= 64 and len(ys2) >= 48 and columns(ys1) != columns(ys2)
    check_scene(rings, det, scene, refs=(0, i2))


def test_both_sides_of_the_direct_table_switch(rings, det):
    b = rings.partners(A_REF)[0]
    below = check_scene(rings, det, one_run(rings, A_REF, b, sector(40.0, MIN_HITS - 1))[0])
    at = check_scene(rings, det, one_run(rings, A_REF, b, sector(40.0, MIN_HITS))[0])
    assert below["n_tables"] == 0 and at["n_tables"] == 1
    assert below["n_lds_atomics"] >= below["n_votes"] and at["n_lds_atomics"] < at["n_votes"]


def test_cold_and_warm_workspace_cast_the_same_atomics(rings, det):
    b = rings.partners(A_REF)[0]
    scene, _ = one_run(rings, A_REF, b, sector(40.0, 64))
    d = torch.from_numpy(scene).cuda()
    ws = Workspace()
    seen = []
    for _ in range(2):
        ws.match_device(det, d.data_ptr(), scene.shape[0], 6, 1.0, 0.05, presampled=True, skip_clustering=True)
        seen.append(ws.results(scene.shape[0])["stats"])
    assert seen[0]["n_lds_atomics"] == seen[1]["n_lds_atomics"] and seen[0]["n_votes"] == seen[1]["n_votes"]
    assert seen[1]["n_retries"] == 0
