"""ppf_prep_clusters on the device against tests/cluster_oracle.py, byte for byte: the labels, the counts, every info record, the
cluster rows with their normals and curvature.  Sizes around the wave, the sort tile and the LDS tile of k_clu_link, one crowded
cell, distances exactly at and one ulp past the tolerance in cells one and two away, long union paths, thousands of mid-sized
components, the ranking rules, non-finite rows, the grid limit, several clouds in one call, repeated and concurrent calls, the
launch and host-sync counts, image boxes, RemovePlanes -> ProposeBoxes -> PrepareFrame -> MatchFrame on the rendered two-bottle
frame, and the C++ demo."""
import os
import subprocess
import threading

import numpy as np
import pytest

import cluster_oracle as CL
import plane_oracle as P
from yolo_ppf_pose_estimation_amd import _capi, synth
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, cluster_clouds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
LAUNCHES = 110                 # 12 kernels of its own, two segmented sorts of 36, one sort of 21, one scan of 5
SMALL = dict(min_size=1)       # the default 100 would reject every small component


def rows6(xyz):
    r = np.zeros((xyz.shape[0], 6), np.float32)
    r[:, :xyz.shape[1]] = xyz
    return r


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def upload(c):
    return DeviceCloud.upload(c if c.shape[0] else np.zeros((0, 3), np.float32))


def blobs(sizes, seed=0, spread=0.004, pitch=0.2):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(size=(n, 3)) * spread + [pitch * i, 0.0, 1.0] for i, n in enumerate(sizes)]).astype(np.float32)


def scattered(n, seed=0):
    """n uniform rows in a cube whose side gives a mean degree of about 1.5 at tolerance 0.02: components of every size"""
    side = (n * 4.0 / 3.0 * np.pi * 0.02 ** 3 / 1.5) ** (1.0 / 3.0) if n else 1.0
    return np.random.default_rng(seed).uniform(0, side, (n, 3)).astype(np.float32)


def assert_cloud(found, info, counts, labels, rows, curv, p, intr=None, image_size=None):
    want_found, want_info, want_counts, want_labels = CL.clusters(rows, p, curv, intr, image_size)
    np.testing.assert_array_equal(labels, want_labels)
    np.testing.assert_array_equal(counts, want_counts)
    assert info.tobytes() == want_info.tobytes(), (info[:4], want_info[:4])
    assert len(found) == len(want_found)
    for got, (want_rows, want_curv) in zip(found, want_found):
        r, c = got.download()
        assert r.shape == want_rows.shape
        np.testing.assert_array_equal(bits(r), bits(want_rows))
        np.testing.assert_array_equal(bits(c), bits(want_curv))
    return want_info, want_counts


def check(clouds, p=None, curvs=None, intr=None, image_size=None):
    """one segmented call on `clouds` ((n, 3) or (n, 6) arrays) against the oracle per cloud; returns (clusters, info, counts, stats)"""
    p = dict(p or {})
    full = [rows6(c) for c in clouds]
    curvs = curvs or [np.zeros(c.shape[0], np.float32) for c in clouds]
    dev = [upload(c) for c in clouds]
    found, info, counts, labels, stats = cluster_clouds(dev, p, intr, image_size, return_info=True, return_labels=True)
    assert info.shape == (len(clouds), p.get("max_clusters", 64)) and stats["n_clouds"] == len(clouds)
    for i, c in enumerate(full):
        assert_cloud(found[i], info[i], counts[i], labels[i], c, curvs[i], p, intr, image_size)
    return found, info, counts, stats


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 4097])
def test_row_counts(n):
    _, _, counts, stats = check([scattered(n, seed=n)], dict(SMALL, max_clusters=256))
    assert counts[0, 2] >= min(n, 1) and stats["n_launches"] == (LAUNCHES if n else 0)
    check([scattered(n, seed=n + 1)], dict(min_size=2, max_size=5, max_clusters=7))


def test_one_crowded_cell():
    cloud = np.tile(np.array([[0.1, 0.2, 0.9]], np.float32), (5000, 1))
    _, info, counts, _ = check([cloud])
    assert list(counts[0]) == [1, 1, 1] and info[0, 0]["n_rows"] == 5000
    # two crowded cells two cells apart that one pair of rows links: the tile loop across cells
    rng = np.random.default_rng(0)
    a = (rng.uniform(0, 0.001, (700, 3)) + [0.0, 0.0, 1.0]).astype(np.float32)
    b = (rng.uniform(0, 0.001, (900, 3)) + [0.03, 0.0, 1.0]).astype(np.float32)
    a[699], b[899] = [0.0055, 0.0, 1.0], [0.0252, 0.0, 1.0]     # 0.0197 apart; every other pair is at least 0.028 apart
    both = np.concatenate([a, b])
    _, info, counts, _ = check([both])
    assert list(counts[0]) == [1, 1, 1]
    _, info, counts, _ = check([np.delete(both, 699, axis=0)])
    assert list(counts[0]) == [2, 2, 2]


TOL = 0.25
CELL = TOL * 0.5773


def test_distances_at_the_tolerance_along_an_axis():
    """tolerance 0.25: a second row exactly 0.25 away (linked) and nextafter(0.25, 1) away (not), to either side, from first
    rows at several places in their cells, so that the second row lands one cell away for some and two for others.  The tested
    coordinate stays below 0.5, where a + 0.25 and a + nextafter(0.25) are exact in float32; pairs are set apart on another axis."""
    far = np.nextafter(np.float32(TOL), np.float32(1))
    for axis in range(3):
        rows, linked = [], 0
        for frac in (0.0, 1.0 / 64, 5.0 / 64, 9.0 / 64, 13.0 / 64):
            for sign in (1.0, -1.0):
                for dist in (np.float32(TOL), far):
                    a = np.zeros(3, np.float32)
                    a[axis], a[(axis + 1) % 3] = frac, 2.0 * (len(rows) // 2)
                    b = a.copy()
                    b[axis] = np.float32(a[axis] + np.float32(sign) * dist)
                    assert abs(float(b[axis]) - float(a[axis])) == float(dist)      # no rounding on the way
                    rows += [a, b]
                    linked += dist == np.float32(TOL)
        cloud = np.array(rows, np.float32)
        cells = np.floor((cloud[:, axis].astype(np.float64) - float(cloud[:, axis].min())) / CELL)
        assert set(np.abs(cells[0::2] - cells[1::2])) == {1.0, 2.0}
        _, _, counts, _ = check([cloud], dict(SMALL, tolerance=TOL, max_clusters=256))
        assert counts[0, 2] == len(rows) - linked
        _, _, counts, _ = check([cloud[np.random.default_rng(axis).permutation(len(rows))]], dict(SMALL, tolerance=TOL, max_clusters=256))
        assert counts[0, 2] == len(rows) - linked


@pytest.mark.parametrize("direction", [(1, 1, 0), (0, 1, -1), (1, 1, 1), (1, -2, 2), (-3, 4, 12)])
def test_distances_at_the_tolerance_along_a_diagonal(direction):
    """no diagonal offset of float32 coordinates is exactly 0.25 long (a sum of three squares of dyadic numbers is 1/16 only
    along an axis), so here the second row is 0.25 along the diagonal, rounded, and its neighbours a few ulps of one coordinate
    to either side: the fp64 predicate links some and not others, and the device has to agree with it on each.  One cloud per
    pair (56 clouds in one call) keeps the coordinates small; a third row, far off, fixes the grid's origin so that the pair's
    place in its cells varies."""
    d = np.array(direction, np.float64) / np.linalg.norm(direction)
    k = int(np.argmax(np.abs(d)))
    clouds = []
    for frac in (0.0, 0.3, 0.6, 0.9):
        for sign in (1.0, -1.0):
            for ulps in range(-3, 4):
                a = (np.array([frac, frac, frac]) * CELL).astype(np.float32)
                b = (a.astype(np.float64) + sign * TOL * d).astype(np.float32)
                for _ in range(abs(ulps)):
                    b[k] = np.nextafter(b[k], np.float32(np.inf if ulps * sign * d[k] > 0 else -np.inf))
                clouds.append(np.array([[-1.0, -1.0, -1.0], a, b], np.float32))
    link = np.array([CL.linked(c[1].astype(np.float64), c[2].astype(np.float64), TOL) for c in clouds])
    assert 0 < link.sum() < link.size
    _, _, counts, _ = check(clouds, dict(SMALL, tolerance=TOL))
    np.testing.assert_array_equal(counts[:, 2], 3 - link)


def chain(n, tol, gap_at=None, fold=None):
    """n rows 0.9 x tol apart along the space diagonal (1, 1, 1); the step before row gap_at is 1.1 x tol.  fold: after every
    `fold` rows the chain takes three steps sideways (so that its runs lie 2.7 x tol apart: not linked) and runs back"""
    d, w = np.ones(3) / np.sqrt(3.0), np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    steps, sign, run = [], 1.0, 0
    while len(steps) < n - 1:
        if fold and run == fold:
            steps += [w * 0.9 * tol] * 3
            sign, run = -sign, 0
        else:
            steps.append(sign * d * 0.9 * tol)
            run += 1
    steps = np.array(steps[:n - 1])
    if gap_at is not None:
        assert abs(abs(steps[gap_at - 1] @ d) - 0.9 * tol) < 1e-12       # a step along the diagonal, not a corner
        steps[gap_at - 1] *= 1.1 / 0.9
    return np.concatenate([np.zeros((1, 3)), np.cumsum(steps, axis=0)]).astype(np.float32)


def test_long_chains():
    """One component with long union paths, in shuffled row order, and the same with one gap: two components.  A straight chain
    of 10,000 rows 0.9 x tolerance apart spans 9,000 cells of the grid, past the 1,024 the stage takes (that call is checked to be
    PPF_ERR_INVALID), so the 10,000 rows run along the diagonal in ten folded runs of 1,000; the straight chain is 1,100 rows."""
    tol = 0.02
    with pytest.raises(_capi.PPFError) as e:
        cluster_clouds([upload(chain(10000, tol))], dict(tolerance=tol))
    assert e.value.status == _capi.PPF_ERR_INVALID and "9000 cells" in str(e.value)
    for n, fold, gap_at in ((10000, 1000, 6000), (1100, None, 600)):
        perm = np.random.default_rng(n).permutation(n)
        _, info, counts, _ = check([chain(n, tol, fold=fold)[perm]], dict(tolerance=tol))
        assert list(counts[0]) == [1, 1, 1] and info[0, 0]["n_rows"] == n
        _, info, counts, _ = check([chain(n, tol, gap_at, fold)[perm]], dict(tolerance=tol))
        assert list(counts[0]) == [2, 2, 2] and sorted(info[0, :2]["n_rows"]) == sorted([gap_at, n - gap_at])
        _, info, counts, _ = check([chain(n, tol, gap_at, fold)], dict(tolerance=tol))        # in chain order: the worst union paths
        assert list(info[0, :2]["first_row"]) == ([0, gap_at] if gap_at >= n - gap_at else [gap_at, 0])


def test_mid_sized_components():
    _, info, counts, _ = check([scattered(20000, seed=3)], dict(SMALL, max_clusters=256))
    assert counts[0, 0] == 256 and counts[0, 1] == counts[0, 2] > 2000 and info[0, 0]["n_rows"] > 20 and info[0, 255]["n_rows"] > 1


def test_ranking():
    cloud = blobs([100, 100, 300, 100, 100, 100], seed=5)
    _, info, counts, _ = check([cloud], dict(min_size=100, max_size=200, max_clusters=3))
    assert list(counts[0]) == [3, 5, 6] and list(info[0]["first_row"]) == [0, 100, 500] and list(info[0]["n_rows"]) == [100] * 3
    _, info, counts, _ = check([cloud], dict(min_size=101))
    assert list(counts[0]) == [1, 1, 6] and info[0, 0]["n_rows"] == 300
    _, info, counts, _ = check([cloud[::-1].copy()])
    assert list(info[0, :6]["n_rows"]) == [300, 100, 100, 100, 100, 100] and list(info[0, 1:6]["first_row"]) == [0, 100, 200, 600, 700]


def test_non_finite_rows():
    cloud = blobs([400, 300], seed=6)
    cloud[::97] = [np.nan, 0.0, 1.0]
    cloud[5::101] = [0.0, np.inf, 0.5]
    cloud[7::103, 2] = -np.inf
    cloud[3] = [1e30, -1e30, 1e30]               # finite: it stretches the grid far past 1,024 cells
    with pytest.raises(_capi.PPFError):
        check([cloud])
    cloud[3] = [np.nan, 1e30, 3e38]              # not finite: out of the bounds
    _, info, counts, _ = check([cloud], dict(min_size=10))
    assert counts[0, 0] == 2 and (info[0, :2]["hi"] < 2).all()
    _, _, counts, _ = check([np.full((300, 3), np.nan, np.float32)], SMALL)
    assert list(counts[0]) == [0, 0, 0]


def test_grid_limit():
    tol = 0.25
    h = tol * 0.5773
    fits = np.array([[0, 0, 0], [0, 0, np.float32(1023.5 * h)]], np.float32)
    _, _, counts, _ = check([fits, fits[:, [2, 0, 1]]], dict(SMALL, tolerance=tol))
    assert list(counts[:, 2]) == [2, 2]
    over = np.array([[0, 0, 0], [np.float32(1024.5 * h), 0, 0]], np.float32)
    with pytest.raises(_capi.PPFError) as e:
        cluster_clouds([upload(fits), upload(over)], dict(SMALL, tolerance=tol), return_info=True)
    assert e.value.status == _capi.PPF_ERR_INVALID and "in[1]" in str(e.value) and "smallest tolerance that fits" in str(e.value)
    smallest = float(np.float32(str(e.value).rsplit(" ", 1)[1]))
    assert tol < smallest < tol * 1.002
    check([over], dict(SMALL, tolerance=smallest))
    with pytest.raises(_capi.PPFError):
        cluster_clouds([upload(over)], dict(SMALL, tolerance=float(np.nextafter(np.float32(smallest), np.float32(0)))))
    for bad in (dict(tolerance=0.0), dict(min_size=0), dict(max_size=-1), dict(max_clusters=0), dict(max_clusters=257), dict(flags=1)):
        with pytest.raises(_capi.PPFError) as e:
            cluster_clouds([upload(fits)], bad)
        assert e.value.status == _capi.PPF_ERR_INVALID
    with pytest.raises(_capi.PPFError):
        cluster_clouds([upload(fits)], dict(tolerence=0.1))


def test_clouds_in_one_call_equal_each_alone():
    sizes = (0, 2, 65, 4097, 1500)
    clouds = [scattered(n, seed=50 + i) for i, n in enumerate(sizes)]
    src = upload(blobs([700, 800], seed=9)).normals(10)      # normals and curvature that are not zero
    rows, curv = src.download()
    assert np.abs(rows[:, 3:]).max() > 0 and curv.max() > 0
    clouds[4], curvs = rows, [np.zeros(n, np.float32) for n in sizes[:4]] + [curv]
    p = dict(min_size=3, max_clusters=40)
    dev = [upload(c) for c in clouds[:4]] + [src]
    found, info, counts, labels, stats = cluster_clouds(dev, p, return_info=True, return_labels=True)
    for i, c in enumerate(clouds):                # each segment against the oracle of that cloud alone
        assert_cloud(found[i], info[i], counts[i], labels[i], rows6(c), curvs[i], p)
        one, info1, counts1, labels1, _ = dev[i].clusters(p, return_info=True, return_labels=True)   # and the device on it alone
        assert info1.tobytes() == info[i].tobytes() and counts1.tobytes() == counts[i].tobytes() and labels1.tobytes() == labels[i].tobytes()
        for a, b in zip(one, found[i]):
            for x, y in zip(a.download(), b.download()):
                np.testing.assert_array_equal(bits(x), bits(y))
    assert counts[3, 0] == 40 and counts[4, 0] == 2
    last = found[4][1].download()
    del found[3], found[3][0]                     # the outputs share one block: the others outlive their siblings
    np.testing.assert_array_equal(bits(found[3][0].download()[0]), bits(last[0]))


def test_launch_and_sync_counts_do_not_depend_on_the_clouds():
    five = [scattered(n, seed=60 + i) for i, n in enumerate((0, 2, 65, 4097, 1500))]
    for p in (dict(SMALL), dict(min_size=5, max_size=9, max_clusters=256, tolerance=0.03)):
        s1 = check([five[3]], p)[3]
        s5 = check(five, p)[3]
        assert (s1["n_launches"], s1["n_host_syncs"]) == (s5["n_launches"], s5["n_host_syncs"]) == (LAUNCHES, 1)
    assert cluster_clouds([], return_info=True)[-1]["n_launches"] == 0
    empty = cluster_clouds([upload(five[0])], return_info=True)[-1]
    assert (empty["n_launches"], empty["n_host_syncs"]) == (0, 0)


def test_repeated_and_concurrent_calls_give_the_same_bytes():
    cloud = upload(scattered(6000, seed=70))
    p = dict(SMALL, max_clusters=100)

    def run():
        f, i, c, l, _ = cloud.clusters(p, return_info=True, return_labels=True)
        return b"".join(k.download()[0].tobytes() for k in f), i.tobytes(), c.tobytes(), l.tobytes()
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


def test_image_boxes():
    cloud = blobs([300, 200, 150], seed=8, pitch=0.3)
    cloud[300:500] -= np.float32([0.0, 0.0, 2.0])        # the second blob lies behind the camera: z < 0, no pixel
    intr, size = (400.0, 400.0, 159.5, 119.5), (240, 320)
    _, info, _, _ = check([cloud], dict(min_size=10), intr=intr, image_size=size)
    assert info[0, 0]["box_xywh"][2] > 0 and not info[0, 1]["box_xywh"].any()
    assert info[0, 2]["box_xywh"][0] + info[0, 2]["box_xywh"][2] == 319      # u = 399 at its centre: clipped at the border
    _, info, _, _ = check([cloud], dict(min_size=10))
    assert not info["box_xywh"].any()
    K = np.array([[400.0, 0, 159.5], [0, 400.0, 119.5], [0, 0, 1]])
    _, info3, _, _ = cluster_clouds([upload(cloud)], dict(min_size=10), K, size, return_info=True)
    assert info3[0, 0]["box_xywh"].tolist() == CL.clusters(cloud, dict(min_size=10), intr=intr, image_size=size)[1][0]["box_xywh"].tolist()


@pytest.fixture(scope="module")
def rendered(bottle):
    from test_gpu_frame import _render_frame
    return _render_frame(bottle)


def test_remove_planes_then_propose_boxes_then_prepare_frame_then_match_frame(rendered, bottle):
    from scipy.spatial import cKDTree
    scene, depth, boxes, K, objs, solid = rendered
    cp = CloudProcessor(scene, depth, [], [], [], 0.05, 0.05)
    cp.LoadSingleModel(bottle, "bottle")
    cp.LoadSingleModel(solid, "box")
    cp.TrainDetector(0.05, 0.05)
    cp.RemovePlanes()
    found = cp.ProposeBoxes(K)
    assert cp.boxes == [(72, 142, 143, 84), (275, 142, 107, 84), (446, 156, 76, 72)]
    assert [len(c) for c in found] == list(cp.cluster_info["n_rows"]) == [8317, 6553, 3140]
    assert (cp.cluster_stats["n_launches"], cp.cluster_stats["n_host_syncs"]) == (LAUNCHES, 1)
    kept = P.remove_planes(scene)[0]
    want = CL.clusters(kept, intr=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), image_size=depth.shape)[1][:3]
    assert cp.cluster_info.tobytes() == want.tobytes()
    cp.PrepareFrame(K, 0.004, 50, 1.0, 30, 0.03)
    assert list(cp.stage_rows[:, 0]) == [8171, 6553, 3120]
    poses = cp.MatchFrame(["bottle", "bottle", "box"])
    for i in (0, 1):
        obj = int(np.argmin([abs(b[0] - cp.boxes[i][0]) for b in boxes]))     # the rendered object under cluster i
        assert obj in (0, 1) and tuple(boxes[obj][:2]) == cp.boxes[i][:2]
        model, T = objs[obj]
        assert poses[i] is not None
        truth = cKDTree(synth.apply_pose(model[::4], T)[:, :3].astype(np.float64))
        d, _ = truth.query(synth.apply_pose(model[::4], poses[i].pose)[:, :3].astype(np.float64))
        print(f"cluster {i}: mean model-to-truth distance {d.mean():.5f} m")
        assert d.mean() < 0.003, (i, d.mean())


@pytest.mark.parametrize("compiler", ["g++"])
def test_cpp_cluster_demo(tmp_path, compiler):
    exe = str(tmp_path / "cluster_demo")
    subprocess.run([compiler, "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "cluster_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    cloud = blobs([500, 120, 300, 40], seed=11, pitch=0.3)[np.random.default_rng(12).permutation(960)]
    (tmp_path / "scene.f32").write_bytes(cloud.tobytes())
    r = subprocess.run([exe, str(tmp_path / "scene.f32"), "960", "0.02", "50", "0", "400", "400", "159.5", "119.5", "240", "320"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = dict(tolerance=0.02, min_size=50)
    found, info, counts, labels = CL.clusters(cloud, p, intr=(400.0, 400.0, 159.5, 119.5), image_size=(240, 320))
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"clusters {counts[0]} valid {counts[1]} components {counts[2]}"
    for k in range(3):
        b = info[k]["box_xywh"]
        assert lines[1 + k] == f"cluster {k}: rows {info[k]['n_rows']} first {info[k]['first_row']} box {b[0]} {b[1]} {b[2]} {b[3]} cloud {found[k][0].shape[0]}"
    assert lines[4] == f"launches {LAUNCHES} host_syncs 1"
    # the PCL-shaped surface: the same components as index lists, ascending inside a cluster
    assert lines[5] == "pcl clusters 3"
    for k in range(3):
        idx = np.flatnonzero(labels == k)
        assert lines[6 + k] == f"pcl cluster {k}: size {idx.size} first {idx[0]} last {idx[-1]} sum {int(idx.sum())}"
