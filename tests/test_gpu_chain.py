"""The small kernels around k_pairs / k_group / k_vote after their fusion: rankings, the in-kernel
zeroing of a batch's scratch, and the clustering chain on every path, each against the CPU oracle.

Clustering is checked on synthetic pose lists whose sizes cross every path boundary: one wave (63 / 64 / 65), one ranking
tile row (1,024 / 1,025), the headline size (2,500), just past the serial kernel's LDS variant (3,601, still below the
4,096 poses up to which the members' kernel scans the sizes and the last kernel ranks the clusters for itself), between that
and the match matrix's limit (6,000: separate k_cluster_offsets and k_rank launches), and past 11,520 (serial assignment).
Vote counts are drawn from a handful of values, so both rankings (poses, clusters) are decided by the index-ascending tie
rule nearly everywhere.

Bounds: cluster count, order and votes are integers and must be equal.  The mean of a cluster is taken in joining order on
both sides (the same fp64 additions in the same order), so the poses are compared at 1e-12 absolute (entries are at most a
few units: a few thousand ulps of slack for the quaternion -> matrix rebuild, the bound tests/test_gpu_edge_cases.py uses);
the two GPU assignment paths must agree bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from yolo_ppf_pose_estimation_amd import _capi, synth
from yolo_ppf_pose_estimation_amd._capi import Pose, lib
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
from yolo_ppf_pose_estimation_amd.device import Workspace

pytestmark = pytest.mark.gpu

POSE_DT = np.dtype([("pose", "f8", (16,)), ("q", "f8", (4,)), ("t", "f8", (3,)), ("angle", "f8"), ("alpha", "f8"),
                    ("residual", "f8"), ("model_index", "u4"), ("num_votes", "u4")])
POS_THR, ROT_THR = 0.05, 0.3
STEP = 1.0 / 10.0


@pytest.fixture(scope="module")
def det(bottle):
    return PPF3DDetector(0.05, 0.05).trainModel(bottle)


@pytest.fixture(scope="module")
def ora(bottle):
    return O.OracleDetector(0.05, 0.05).train_model(bottle)


@pytest.fixture(scope="module")
def crop(bottle):
    return synth.make_scene(bottle, n_points=5030, seed=33)[0]  # 503 reference points: not a multiple of 64 (nor of 16)


@pytest.fixture(scope="module")
def oracle_crop(ora, crop):
    ora.set_search_params(-1.0, -1.0, False)
    ora.set_policy()
    return ora.match(crop, relative_scene_sample_step=STEP, presampled=True, cluster=True)


def make_poses(n, seed):
    """n pose records around about n / 3 centres: members of a centre lie well inside both thresholds of it, centres are
    spread so that many (not all) are apart; votes from {1 .. 6}, so ties are the rule."""
    assert POSE_DT.itemsize == C.sizeof(Pose) == C.sizeof(O.OraclePose)
    rng = np.random.default_rng(seed)
    k = max(1, n // 3)
    c_t = rng.uniform(-0.4, 0.4, size=(k, 3))
    c_axis = rng.normal(size=(k, 3)); c_axis /= np.linalg.norm(c_axis, axis=1, keepdims=True)
    c_ang = rng.uniform(0.2, 2.8, size=k)
    who = rng.integers(0, k, size=n)
    t = c_t[who] + rng.uniform(-0.3, 0.3, size=(n, 3)) * POS_THR
    axis = c_axis[who] + rng.normal(size=(n, 3)) * 0.02
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = c_ang[who] + rng.uniform(-0.3, 0.3, size=n) * ROT_THR
    rec = np.zeros(n, dtype=POSE_DT)
    q = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], axis=1)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    P = np.zeros((n, 4, 4)); P[:, :3, :3] = R; P[:, :3, 3] = t; P[:, 3, 3] = 1.0
    rec["pose"] = P.reshape(n, 16); rec["q"] = q; rec["t"] = t; rec["angle"] = ang
    rec["model_index"] = rng.integers(0, 2000, size=n)
    rec["num_votes"] = rng.integers(1, 7, size=n)
    return rec


def oracle_cluster(ora, rec, num_poses, weighted=False, rot_relative=False):
    ora.set_search_params(POS_THR, ROT_THR, weighted)
    ora.set_policy(rot_relative=rot_relative)
    n = rec.shape[0]
    src = (O.OraclePose * n).from_buffer_copy(rec.tobytes())
    out = (O.OraclePose * n)()
    nf = O.lib().oracle_cluster(ora.h, src, n, num_poses, out, n)
    return np.frombuffer(out, dtype=POSE_DT)[:nf].copy()


def device_cluster(det, rec, num_poses, weighted=False, rot_relative=False, serial=False):
    """ppf_cluster_poses_device on a workspace (optionally forced to the serial assignment); every cluster comes back."""
    import torch
    det.setSearchParams(POS_THR, ROT_THR, weighted)
    det.setPolicy(rot_metric_relative=rot_relative)
    n = rec.shape[0]
    ws = Workspace()
    if serial:
        ws.set_option(_capi.PPF_OPT_CLUSTER_SERIAL, 1)
    d = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.float64).copy()).cuda()
    blk = ws.cluster_device(det, d.data_ptr(), n, num_poses, top_k=n)
    torch.cuda.synchronize()
    out = np.frombuffer(blk.cpu().numpy().tobytes(), dtype=POSE_DT)
    nf = int(np.count_nonzero(out["num_votes"]))
    assert not out["num_votes"][nf:].any()
    return out[:nf].copy()


def host_cluster(det, rec, num_poses, weighted=False, rot_relative=False):
    """ppf_cluster_poses, the host-buffer entry"""
    det.setSearchParams(POS_THR, ROT_THR, weighted)
    det.setPolicy(rot_metric_relative=rot_relative)
    n = rec.shape[0]
    src = (Pose * n).from_buffer_copy(rec.tobytes())
    out = (Pose * n)()
    nout = C.c_int(0)
    mp = det._params(1.0, 0.05, True)
    _capi.check(lib().ppf_cluster_poses(det._model.ptr, src, n, num_poses, C.byref(mp), out, n, C.byref(nout)))
    return np.frombuffer(out, dtype=POSE_DT)[:nout.value].copy()


def assert_clusters(got, want, exact=False):
    assert got.shape[0] == want.shape[0]
    np.testing.assert_array_equal(got["num_votes"], want["num_votes"])
    np.testing.assert_array_equal(got["model_index"], want["model_index"])  # the cluster's first member: the order of ties
    if exact:
        for f in ("pose", "q", "t", "angle"):
            np.testing.assert_array_equal(got[f], want[f])
    else:
        for f in ("pose", "q", "t", "angle"):
            np.testing.assert_allclose(got[f], want[f], rtol=0, atol=1e-12)


@pytest.fixture(autouse=True)
def _restore(det, ora):
    yield
    det.setSearchParams(-1, -1, False)
    det.setPolicy()
    ora.set_search_params(-1.0, -1.0, False)
    ora.set_policy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 2500, 3601, 6000, 12000])
def test_clustering_across_the_path_boundaries(det, ora, n):
    rec = make_poses(n, seed=n)
    want = oracle_cluster(ora, rec, n)
    assert want.shape[0] >= 1 and (n < 64 or want.shape[0] < n)            # clusters with several members
    assert n < 64 or np.unique(want["num_votes"]).size < want.shape[0]      # cluster votes tie as well
    got = device_cluster(det, rec, n)
    assert_clusters(got, want)
    if n <= 6000:  # the forced serial assignment (k_cluster_assign in LDS up to 3,600 poses, from global memory above)
        assert_clusters(device_cluster(det, rec, n, serial=True), got, exact=True)
    # the reference drops the lowest-voted pose when the stride does not divide the row count: num_poses < n
    if n > 1:
        assert_clusters(device_cluster(det, rec, n - 1), oracle_cluster(ora, rec, n - 1))


@pytest.mark.parametrize("n", [65, 1025, 2500, 6000])
@pytest.mark.parametrize("weighted", [False, True])
def test_clustering_with_both_rotation_metrics(det, ora, n, weighted):
    rec = make_poses(n, seed=1000 + n)
    for rel in (False, True):
        want = oracle_cluster(ora, rec, n, weighted=weighted, rot_relative=rel)
        assert_clusters(device_cluster(det, rec, n, weighted=weighted, rot_relative=rel), want)
    assert_clusters(host_cluster(det, rec, n, weighted=weighted), oracle_cluster(ora, rec, n, weighted=weighted))


def test_all_votes_equal_leaves_everything_to_the_index_rule(det, ora):
    rec = make_poses(2500, seed=5)
    rec["num_votes"] = 7
    want = oracle_cluster(ora, rec, 2500)
    assert_clusters(device_cluster(det, rec, 2500), want)
    assert_clusters(device_cluster(det, rec, 2500, serial=True), want)


def _run(det, crop, ws=None, **kw):
    import torch
    ws = ws or Workspace()
    d = torch.from_numpy(crop).cuda()
    ws.match_device(det, d.data_ptr(), crop.shape[0], 6, STEP, 0.05, presampled=True, **kw)
    return ws.results(crop.shape[0])


def _assert_match(res, want, poses=True):
    assert res["n_ref"] == want["n_ref"]
    np.testing.assert_array_equal(res["triples"], want["triples"])
    assert res["stats"]["n_votes"] == int(want["votes_per_ref"].sum())
    assert res["stats"]["n_pairs"] == int(want["pairs_per_ref"].sum())
    if poses:
        assert len(res["poses"]) == want["n_final"] > 1
        for g, w in zip(res["poses"], want["poses"]):
            assert g.numVotes == w["num_votes"]
            np.testing.assert_allclose(g.pose, w["pose"], rtol=0, atol=1e-12)


def test_match_with_a_reference_count_that_fills_no_wave(det, crop, oracle_crop):
    assert oracle_crop["n_ref"] == 503 and oracle_crop["n_ref"] % 64 != 0
    _assert_match(_run(det, crop), oracle_crop)


def test_cold_workspace_then_warm(det, crop, oracle_crop):
    """The first call of a workspace counts its hits in a pass of its own (which uses the cursors before k_frames clears them),
    the second sizes its pools from the first: same answer, and the second runs without a repeat."""
    ws = Workspace()
    cold = _run(det, crop, ws)
    warm = _run(det, crop, ws)
    _assert_match(cold, oracle_crop)
    _assert_match(warm, oracle_crop)
    assert warm["stats"]["n_retries"] == 0
    for k in ("n_hits", "n_tables", "n_lds_atomics"):
        assert cold["stats"][k] == warm["stats"][k]


def _far_rows(n, seed):
    """n ordinary points on a line tens of metres from the crop and metres from each other: a reference point among them
    pairs with everything at distances far beyond the model's, so it finds (next to) no bucket."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 6), dtype=np.float32)
    rows[:, 0] = 80.0 + 3.0 * np.arange(n)
    rows[:, 1] = -40.0
    nn = rng.normal(size=(n, 3)); nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    rows[:, 3:] = nn
    return rows


def test_several_batches_keep_the_overflow_word(det, ora, crop, oracle_crop):
    """k_frames clears the cursors of every batch but must leave the overflow word to the later batches of a call.  The crop is
    followed by 160 far-away rows, so that the call's last batch is ONE reference point (518 of 519, batches of 37) among them
    with so few hits that it cannot overflow the smallest pools there are, while pools sized for a three-hundredth of the hits
    overflow in every batch of the crop's own reference points: unless the flag survives the last batch's k_frames, the call is
    not repeated and its votes fall short."""
    ws = Workspace()
    ws.set_option(_capi.PPF_OPT_BATCH_REFS, 37)
    res = _run(det, crop, ws)
    assert res["stats"]["n_batches"] == -(-503 // 37)
    _assert_match(res, oracle_crop)

    cloud = np.concatenate([crop, _far_rows(160, 7)]).astype(np.float32)
    want = ora.match(cloud, relative_scene_sample_step=STEP, presampled=True, cluster=True)
    assert want["n_ref"] == 519 == 14 * 37 + 1
    # With the fraction below every pool of a batch is at its least size: 64 * 37 hits (+ 4,096 sorted, more raw), 64 * 37 + 1,024
    # runs, over 256 count tables.  A hit casts at least one vote, a run has at least one hit, a table at least 24: the last
    # batch's single reference point fits them all.
    assert int(want["votes_per_ref"][518]) < 64 * 37 + 1024
    ws2 = Workspace()
    ws2.set_option(_capi.PPF_OPT_BATCH_REFS, 37)
    ws2.set_option(_capi.PPF_OPT_HIT_FRACTION, 0.0005)
    res2 = _run(det, cloud, ws2)
    assert res2["stats"]["n_batches"] == 15 and res2["stats"]["n_retries"] >= 1
    _assert_match(res2, want)
    one = _run(det, cloud)
    assert one["stats"]["n_batches"] == 1
    for g, w in zip(res2["poses"], one["poses"]):
        assert g.numVotes == w.numVotes and np.array_equal(g.pose, w.pose)


def test_odd_reference_frame_in_one_batch_of_several(det, ora, crop):
    """The "odd values" word is raised by writing the number of the k_frames launch.  Here the paired points (a separate edge
    cloud) are ordinary and ONE reference point, in the third of six batches, has an infinite coordinate: only that batch's
    k_frames raises the word, after two launches that left it alone, and the batch must honour it (the reference counts none of
    that point's pairs: k_pairs_odd takes them off the totals again).  Then a clean call on the same workspace and the odd one again: the word must
    be raised anew by a later launch's number.  (A stale number honoured by mistake would only make k_group check hits that
    all pass: no output can show it, so that side is not tested.)"""
    surf = crop.copy()
    surf[2500, 0] = np.inf  # reference point 250: batch 2 of batches of 100
    edge = crop.copy()
    want = ora.match(surf, edge=edge, relative_scene_sample_step=STEP, presampled=True, cluster=True)
    clean = ora.match(crop, edge=edge, relative_scene_sample_step=STEP, presampled=True, cluster=True)
    assert int(want["pairs_per_ref"][250]) == 0 and int(clean["pairs_per_ref"][250]) == 5029  # the odd frame's pairs are not counted

    def run(ws, cloud):
        import torch
        d = torch.from_numpy(cloud).cuda()
        e = torch.from_numpy(edge).cuda()
        ws.match_device(det, d.data_ptr(), cloud.shape[0], 6, STEP, 0.05, presampled=True, d_edge_ptr=e.data_ptr(),
                        ne=edge.shape[0], estride=6)
        return ws.results(cloud.shape[0])

    ws = Workspace()
    ws.set_option(_capi.PPF_OPT_BATCH_REFS, 100)
    first = run(ws, surf)
    assert first["stats"]["n_batches"] == 6
    _assert_match(first, want)
    _assert_match(run(ws, crop), clean)
    _assert_match(run(ws, surf), want)


def test_skip_clustering_shards_add_up(det, crop, oracle_crop):
    """Three shards of the reference points (ref_offset / ref_stride, skip_clustering), merged in reference order and clustered
    by ppf_cluster_poses_device, are the unsharded match."""
    import torch
    full = _run(det, crop)
    _assert_match(full, oracle_crop)
    n = full["n_ref"]
    merged = np.zeros(n, dtype=POSE_DT)
    tri = np.zeros((n, 3), dtype=np.uint32)
    votes = pairs = 0
    for off in range(3):
        ws = Workspace()
        part = _run(det, crop, ws, ref_offset=off, ref_stride=3, skip_clustering=True)
        assert part["poses"] == [] and part["n_ref"] == len(range(off, n, 3))
        blk = ws.device_pose_block(part["n_ref"])
        torch.cuda.synchronize()
        merged[off::3] = np.frombuffer(blk.cpu().numpy().tobytes(), dtype=POSE_DT)
        tri[off::3] = part["triples"]
        votes += part["stats"]["n_votes"]; pairs += part["stats"]["n_pairs"]
    np.testing.assert_array_equal(tri, oracle_crop["triples"])
    assert votes == full["stats"]["n_votes"] and pairs == full["stats"]["n_pairs"]
    d = torch.from_numpy(np.frombuffer(merged.tobytes(), dtype=np.float64).copy()).cuda()
    ws = Workspace()
    det.setSearchParams(-1, -1, False)
    blk = ws.cluster_device(det, d.data_ptr(), n, crop.shape[0] // 10, top_k=n)
    torch.cuda.synchronize()
    got = np.frombuffer(blk.cpu().numpy().tobytes(), dtype=POSE_DT)
    got = got[: int(np.count_nonzero(got["num_votes"]))]
    assert got.shape[0] == len(full["poses"])
    for g, w in zip(got, full["poses"]):
        assert int(g["num_votes"]) == w.numVotes
        np.testing.assert_array_equal(g["pose"].reshape(4, 4), w.pose)


def test_batch_repeats_a_match_whose_pools_were_too_small(det, bottle):
    """The overflow retry inside ppf_batch_run.  One lane, one model, two crops: the first is 2,000 points scattered over a box
    a hundred model diameters wide, where next to no pair is a hit, so the lane's cold count learns the least hit fraction; the
    second, an ordinary scene of 2,000 points, then runs with pools far too small, raises the overflow word and is repeated
    with grown pools after the lane has drained.  Both crops must come out as a match of that crop alone does."""
    from yolo_ppf_pose_estimation_amd.device import BatchMatcher
    rng = np.random.default_rng(5)
    sparse = np.zeros((2000, 6), dtype=np.float32)
    sparse[:, :3] = rng.uniform(-15.0, 15.0, size=(2000, 3))
    nn = rng.normal(size=(2000, 3))
    sparse[:, 3:] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
    scene = synth.make_scene(bottle, n_points=2000, seed=21)[0]
    crops = [sparse, scene]
    top_k = 5
    res = BatchMatcher(lanes=1).run([det], crops, STEP, 0.05, presampled=True, top_k=top_k)
    assert res["n_matches"] == 2 and res["n_retries"] >= 1
    for c, cloud in enumerate(crops):
        want = det.match(cloud, STEP, 0.05, presampled=True)[:top_k]
        got = res["poses"][c][0]
        assert [p.numVotes for p in got] == [p.numVotes for p in want], c
        for g, w in zip(got, want):
            np.testing.assert_allclose(g.pose, w.pose, rtol=0, atol=1e-9)
    assert len(res["poses"][1][0]) >= 1 and res["poses"][1][0][0].numVotes > 0
