"""ppf_prep_planes / ppf_prep_planes_apply on the device against tests/plane_oracle.py, byte for byte: the kept rows with their
normals and curvature, the labels and every info field, the doubles included.  Sizes around the boundaries of the sum tree
(64, 4,096) and of the hypothesis blocks (64, 256), every flag, non-finite rows, several clouds in one call, repeated and
concurrent calls, the launch and host-sync counts, the reference's frame, and RemovePlanes in front of PrepareFrame and
MatchFrame on the rendered two-bottle frame."""
import os
import subprocess
import threading

import numpy as np
import pytest

import oracle_lib as OL
import plane_oracle as P
import prep_data as D
from yolo_ppf_pose_estimation_amd import synth
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, remove_planes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
SMALL = dict(min_inliers=3)   # the default 100 would reject every small cloud


def rows6(xyz):
    r = np.zeros((xyz.shape[0], 6), np.float32)
    r[:, :xyz.shape[1]] = xyz
    return r


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mixed(n, seed=0, noise=0.0005):
    """n rows: four fifths a plane with half a millimetre of noise, the rest a sphere, shuffled"""
    k = (4 * n) // 5
    plane, _ = D.plane_cloud(n=k, seed=seed, noise=noise)
    sphere, _ = D.sphere_cloud(n=n - k, seed=seed + 1)
    return np.concatenate([plane, sphere])[np.random.default_rng(seed + 2).permutation(n)]


def stacked(seed=0):
    """three planes of 1,200 rows and a sphere of 800, shuffled"""
    planes = [D.plane_cloud(n=1200, seed=seed + s, normal=nv, offset=o, noise=0.0005)[0]
              for s, nv, o in ((0, (0, 0, -1.0), 0.9), (1, (0, -1.0, -0.2), 0.5), (2, (1.0, 0.1, -0.3), 0.45))]
    return np.concatenate(planes + [D.sphere_cloud(n=800, seed=seed + 3)[0]])[np.random.default_rng(seed + 4).permutation(4400)]


def assert_cloud(got_cloud, got_info, got_labels, rows, curv, p):
    want_rows, want_curv, want_info, want_labels = P.remove_planes(rows, p, curv)
    np.testing.assert_array_equal(got_labels, want_labels)
    assert got_info.tobytes() == want_info.tobytes(), (got_info, want_info)
    r, c = got_cloud.download()
    assert r.shape == want_rows.shape
    np.testing.assert_array_equal(bits(r), bits(want_rows))
    np.testing.assert_array_equal(bits(c), bits(want_curv))
    return want_info


def check(clouds, p=None, curvs=None):
    """one segmented call on `clouds` ((n, 3) or (n, 6) arrays) against the oracle per cloud; returns (device clouds, info, stats)"""
    p = dict(p or {})
    full = [rows6(c) for c in clouds]
    curvs = curvs or [np.zeros(c.shape[0], np.float32) for c in clouds]
    dev = [DeviceCloud.upload(c) if c.shape[0] else DeviceCloud.upload(np.zeros((0, 3), np.float32)) for c in clouds]
    kept, info, labels, stats = remove_planes(dev, p, return_info=True, return_labels=True)
    assert info.shape == (len(clouds), p.get("max_planes", 1)) and stats["n_clouds"] == len(clouds) and stats["n_host_syncs"] <= 2
    for i, c in enumerate(full):
        assert_cloud(kept[i], info[i], labels[i], c, curvs[i], p)
    return kept, info, stats


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 4096, 4097, 10000])
def test_row_counts_around_the_tree_boundaries(n):
    for flags in (0, P.NO_REFIT):
        _, info, _ = check([mixed(n, seed=n)], dict(SMALL, flags=flags))
        assert info[0, 0]["status"] == (P.NONE if n < 3 else P.REMOVED)


@pytest.mark.parametrize("h,n", [(1, 1500), (63, 1500), (64, 1500), (65, 1500), (256, 1500), (257, 1500), (4096, 300)])
def test_hypothesis_counts(h, n):
    _, info, _ = check([mixed(n, seed=h)], dict(SMALL, n_hypotheses=h, seed=7))
    assert info[0, 0]["status"] == (P.REMOVED if h > 1 else P.REJECTED) and 0 <= info[0, 0]["hypothesis"] < h   # the one hypothesis of h = 1 misses


@pytest.mark.parametrize("planes", [1, 2, 4])
@pytest.mark.parametrize("flags", [0, P.NO_REFIT, P.REMOVE_BEHIND, P.NO_REFIT | P.REMOVE_BEHIND])
def test_stacked_planes_every_flag(planes, flags):
    kept, info, _ = check([stacked()], dict(max_planes=planes, flags=flags))
    assert (info[0]["status"] == P.REMOVED).all() and (info[0]["n_inliers"][:3] == 1200).all()   # a fourth plane: a slab of the sphere
    assert (info[0]["refit"][info[0]["status"] == P.REMOVED] == (0 if flags & P.NO_REFIT else 1)).all()


def test_non_finite_rows_stay():
    cloud = mixed(3000, seed=21)
    cloud[::97] = [np.nan, 0.0, 1.0]
    cloud[5::101] = [0.0, np.inf, 0.5]
    cloud[7::103, 2] = -np.inf
    for flags in (0, P.REMOVE_BEHIND):
        kept, info, _ = check([cloud], dict(flags=flags, max_planes=2))
        bad = ~np.isfinite(cloud).all(axis=1)
        assert info[0, 0]["status"] == P.REMOVED and (~np.isfinite(kept[0].xyz()).all(axis=1)).sum() == bad.sum()
    # nothing but non-finite rows, and identical rows: every hypothesis is invalid
    for cloud in (np.full((500, 3), np.nan, np.float32), np.tile(np.array([[0.1, 0.2, 0.9]], np.float32), (500, 1))):
        kept, info, _ = check([cloud], dict(n_hypotheses=64))
        assert info[0, 0]["status"] == P.REJECTED and info[0, 0]["n_hyp_inliers"] == 0 and len(kept[0]) == 500


def test_an_exact_plane_leaves_nothing():
    cloud, _ = D.plane_cloud(n=5000, seed=30, noise=0.0)
    kept, info, _ = check([cloud], dict(max_planes=2))
    assert len(kept[0]) == 0 and info[0, 0]["n_inliers"] == 5000 and list(info[0]["status"]) == [P.REMOVED, P.NONE]
    assert kept[0].download()[0].shape == (0, 6)


def test_normals_and_curvature_are_carried():
    src = DeviceCloud.upload(mixed(3000, seed=40)).normals(10)
    rows, curv = src.download()
    assert np.abs(rows[:, 3:]).max() > 0 and curv.max() > 0
    kept, info, labels, _ = src.remove_planes(dict(max_planes=2), return_info=True, return_labels=True)
    assert info.shape == (2,) and labels.shape == (3000,)
    assert_cloud(kept, info, labels, rows, curv, dict(max_planes=2))
    # apply: the planes taken out of the cloud itself give the same bytes, out of another cloud what the oracle keeps
    again = src.apply_planes(info, dict(max_planes=2))
    for a, b in zip(again.download(), kept.download()):
        np.testing.assert_array_equal(bits(a), bits(b))
    other = rows6(mixed(2000, seed=40))
    for flags in (0, P.REMOVE_BEHIND):
        got = DeviceCloud.upload(other).apply_planes(info, dict(flags=flags)).rows()
        np.testing.assert_array_equal(bits(got), bits(other[P.apply_planes(other, info, dict(flags=flags))]))
    assert len(DeviceCloud.upload(other).apply_planes(info[:0])) == 2000


def test_clouds_in_one_call_equal_each_alone():
    sizes = (0, 2, 65, 4097, 1500)
    clouds = [mixed(n, seed=50 + i) for i, n in enumerate(sizes)]
    p = dict(SMALL, max_planes=2)
    kept, info, stats = check(clouds, p)          # each segment against the oracle of that cloud alone
    for i, c in enumerate(clouds):                # and against the device on that cloud alone
        one, info1, labels1, _ = DeviceCloud.upload(c).remove_planes(p, return_info=True, return_labels=True)
        assert info1.tobytes() == info[i].tobytes()
        for a, b in zip(one.download(), kept[i].download()):
            np.testing.assert_array_equal(bits(a), bits(b))
    del kept[3]                                    # the outputs share one block: the others outlive a sibling
    assert len(kept[3]) == len(kept[3].rows())


def test_launch_and_sync_counts_do_not_depend_on_the_clouds():
    five = [mixed(n, seed=60 + i) for i, n in enumerate((0, 2, 65, 4097, 1500))]
    for planes in (1, 3):
        for flags, per_round in ((0, 16), (P.NO_REFIT, 10), (P.REMOVE_BEHIND, 16)):
            p = dict(SMALL, max_planes=planes, flags=flags)
            s1 = check([five[3]], p)[2]
            s5 = check(five, p)[2]
            assert (s1["n_launches"], s1["n_host_syncs"]) == (s5["n_launches"], s5["n_host_syncs"]) == (2 + per_round * planes, 1)
    assert remove_planes([], return_info=True)[-1]["n_launches"] == 0


def test_repeated_and_concurrent_calls_give_the_same_bytes():
    cloud = DeviceCloud.upload(stacked(seed=70))
    p = dict(max_planes=3)

    def run():
        k, i, l, _ = cloud.remove_planes(p, return_info=True, return_labels=True)
        return k.download()[0].tobytes(), i.tobytes(), l.tobytes()
    first = run()
    assert run() == first
    got = [None, None]

    def work(j):
        got[j] = [run() for _ in range(3)]
    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(r == first for g in got for r in g)


def test_reference_frame_two_planes():
    xyz, _, _, _ = D.c1_frame()
    assert xyz.shape[0] == 166718
    p = dict(n_hypotheses=256, max_planes=2)
    kept, info, stats = check([xyz], p)
    assert list(info[0]["status"]) == [P.REMOVED, P.REMOVED]
    # the table: n ~ (0.002, -0.856, -0.518), d ~ 0.714, about a quarter of the rows
    assert np.abs(info[0, 0]["n"] - [0.002, -0.856, -0.518]).max() < 0.01 and abs(info[0, 0]["d"] - 0.714) < 0.005
    assert 40000 < info[0, 0]["n_inliers"] < 46000 and 20000 < info[0, 1]["n_inliers"] < 30000


@pytest.fixture(scope="module")
def rendered(bottle):
    from test_gpu_frame import _render_frame
    return _render_frame(bottle)


def test_remove_planes_then_prepare_frame_then_match_frame(rendered, bottle):
    from scipy.spatial import cKDTree
    scene, depth, boxes, K, objs, solid = rendered
    labels = ["bottle", "bottle", "box"]
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    runs = {}
    for remove in (False, True):
        cp = CloudProcessor(scene, depth, boxes, [39, 39, 73], [0, 1, 2], 0.05, 0.05)
        cp.LoadSingleModel(bottle, "bottle")
        cp.LoadSingleModel(solid, "box")
        cp.TrainDetector(0.05, 0.05)
        if remove:
            cp.RemovePlanes()
            assert cp.plane_info[0]["status"] == P.REMOVED and cp.plane_info[0]["n_inliers"] == 212390 and len(cp.scene) == 18010
            assert cp.plane_stats["n_host_syncs"] <= 2
        cp.PrepareFrame(K, 0.004, 50, 1.0, 30, 0.03)
        runs[remove] = (cp.MatchFrame(labels), [list(f) for f in cp.frame_poses], cp.stage_rows.copy())
    poses, ranked, stage_rows = runs[True]
    kept_scene = P.remove_planes(scene)[0]
    want_crop = [kept_scene[OL.prep_crop(kept_scene, b, depth, intr)[0]].shape[0] for b in boxes]
    assert list(stage_rows[:, 0]) == want_crop and want_crop[:2] == [6553, 8171]
    for i in (0, 1):
        model, T = objs[i]
        assert poses[i] is not None
        truth = cKDTree(synth.apply_pose(model[::4], T)[:, :3].astype(np.float64))
        d, _ = truth.query(synth.apply_pose(model[::4], poses[i].pose)[:, :3].astype(np.float64))
        assert d.mean() < 0.003, (i, d.mean())
        with_votes, without_votes = ranked[i][0].numVotes, runs[False][1][i][0].numVotes
        print(f"bottle {i}: best pose {with_votes} votes with the plane removed, {without_votes} without; crop rows {stage_rows[i, 0]} / {runs[False][2][i, 0]}")
        assert with_votes > without_votes


@pytest.mark.parametrize("compiler", ["g++"])
def test_cpp_facade_remove_planes(tmp_path, compiler):
    exe = str(tmp_path / "plane_remove_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "plane_remove_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    cloud, other = stacked(seed=80), mixed(1000, seed=81)
    (tmp_path / "scene.f32").write_bytes(cloud.tobytes())
    (tmp_path / "other.f32").write_bytes(other.tobytes())
    r = subprocess.run([exe, str(tmp_path / "scene.f32"), "4400", "4", "128", "0.004", str(tmp_path / "other.f32"), "1000"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = dict(max_planes=4, n_hypotheses=128, distance_threshold=0.004)
    kept, _, info, labels = P.remove_planes(cloud, p)
    lines = r.stdout.strip().splitlines()
    for k in range(4):
        f = lines[k].split()
        assert [int(f[j]) for j in (3, 5, 7, 9, 11, 13)] == [info[k][n] for n in ("status", "hypothesis", "n_rows", "n_inliers", "n_behind", "refit")]
        assert np.abs(np.array([float(v) for v in f[15:18]]) - info[k]["n"]).max() < 1e-8 and abs(float(f[19]) - info[k]["d"]) < 1e-8
    assert lines[4] == f"kept {kept.shape[0]} of 4400 removed {(labels != 0).sum()}"
    assert lines[5] == f"companion kept {P.apply_planes(other, info, p).sum()} of 1000"
    assert lines[6] == f"launches {2 + 16 * 4} host_syncs 1"
