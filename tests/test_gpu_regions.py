"""ppf_prep_regions on the device against tests/region_oracle.py, byte for byte: the labels, the counts, every info record, the
region rows with their normals and curvature.  Sizes around the wave, the sort tile and the LDS tile of k_reg_link, crowded
cells on both sides of a tile, two regions interleaved in one cell, a link two cells away, the three thresholds, the border
rules, non-finite values, the unoriented flag, two planes that meet in an edge, long union paths, the ranking rules, the grid
limit, several clouds in one call, the launch and host-sync counts, repeated and concurrent calls, image boxes, ppf_prep_clusters
where the two specifications coincide, the rendered frame from its depth image, and the C++ demo.  Every input is a valid cloud."""
import os
import subprocess
import threading

import numpy as np
import pytest

import region_cases as RC
import region_oracle as R
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, cluster_clouds, region_clouds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
LAUNCHES = 111                 # ppf_prep_clusters' 110 (test_gpu_clusters.py) and k_reg_attach
SMALL = dict(min_size=1, max_regions=256)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def upload(rows, curv):
    return DeviceCloud.upload(rows.reshape(-1, 6) if rows.shape[0] else np.zeros((0, 6), np.float32), curvature=curv)


def assert_cloud(found, info, counts, labels, rows, curv, p, intr=None, image_size=None):
    want_found, want_info, want_counts, want_labels = R.regions(rows, p, curv, intr, image_size)
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


def check(clouds, p=None, intr=None, image_size=None):
    """one segmented call on `clouds` ((rows (n, 6), curvature (n,)) pairs) against the oracle per cloud; returns (regions, info,
    counts, labels, stats)"""
    p = dict(p or {})
    dev = [upload(r, c) for r, c in clouds]
    found, info, counts, labels, stats = region_clouds(dev, p, intr, image_size, return_info=True, return_labels=True)
    assert info.shape == (len(clouds), p.get("max_regions", 64)) and counts.shape == (len(clouds), 4) and stats["n_clouds"] == len(clouds)
    for i, (r, c) in enumerate(clouds):
        assert_cloud(found[i], info[i], counts[i], labels[i], r, c, p, intr, image_size)
    return found, info, counts, labels, stats


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_row_counts(n):
    _, _, counts, _, stats = check([RC.patches(n, seed=n)], dict(SMALL, tolerance=0.02))
    assert counts[0, 2] >= min(n, 1) - (n == 1) and stats["n_launches"] == (LAUNCHES if n else 0)
    assert n < 63 or (counts[0, 3] > 0 and counts[0, 2] > 3)
    check([RC.patches(n, seed=n + 1)], dict(tolerance=0.02, min_size=2, max_size=5, max_regions=7))
    check([RC.random_cloud(n, seed=n, side=0.3)], dict(SMALL, tolerance=0.03, normal_cos=0.2, flags=n & 1))


def crowded(n, seed, interleaved=False):
    """n rows inside one cell of the grid at tolerance 0.02: a cube of 2 mm at the grid's origin, a cell being 11.5 mm.  Three
    normals and a fifth of the rows border rows, or (interleaved) two normals in turn and every row smooth"""
    rng = np.random.default_rng(seed)
    rows = RC.rows6(rng.uniform(0, 0.002, (n, 3)) + [0.1, 0.2, 0.9])
    if interleaved:
        rows[1::2, 3:] = RC.X
        return rows, RC.smooth(n)
    rows[:, 3:] = np.array([RC.Z, RC.X, (0.0, 0.6, 0.8)], np.float32)[rng.integers(0, 3, n)]
    return rows, np.where(rng.uniform(size=n) < 0.2, RC.ROUGH, np.float32(0.0)).astype(np.float32)


@pytest.mark.parametrize("n", [256, 257])
def test_one_crowded_cell_at_the_tile_boundary(n):
    _, info, counts, _, _ = check([crowded(n, n)], dict(SMALL, tolerance=0.02))
    assert list(counts[0, :3]) == [3, 3, 3] and info[0, :3]["n_rows"].sum() == n
    rows, curv = crowded(n, n)
    curv[:] = 0
    rows[:, 3:] = RC.Z
    rows[n - 1, 3:] = RC.X          # the last row alone: the one past the tile when n is 257
    _, info, counts, _, _ = check([(rows, curv)], dict(SMALL, tolerance=0.02))
    assert list(info[0, :2]["n_rows"]) == [n - 1, 1] and info[0, 1]["first_row"] == n - 1


def test_two_regions_interleaved_in_one_cell():
    _, info, counts, labels, _ = check([crowded(600, 3, interleaved=True)], dict(SMALL, tolerance=0.02))
    assert list(counts[0]) == [2, 2, 2, 0] and list(info[0, :2]["n_rows"]) == [300, 300] and list(info[0, :2]["first_row"]) == [0, 1]
    assert (labels[0][0::2] == 0).all() and (labels[0][1::2] == 1).all()


def test_a_link_two_cells_away_in_the_last_tile():
    _, info, counts, _, _ = check([RC.two_cells_apart()], dict(tolerance=0.02))
    assert list(counts[0]) == [1, 1, 1, 0] and info[0, 0]["n_rows"] == 1600
    _, info, counts, _, _ = check([RC.two_cells_apart(disagree=True)], dict(tolerance=0.02))
    assert list(counts[0]) == [2, 2, 2, 0] and list(info[0, :2]["n_rows"]) == [900, 700]
    rows, curv = RC.two_cells_apart()
    _, _, counts, _, _ = check([(np.delete(rows, 699, axis=0), curv[1:])], dict(tolerance=0.02))
    assert list(counts[0]) == [2, 2, 2, 0]


def test_thresholds():
    rows, curv, cos, linked = RC.cosine_threshold()
    for flags, want in ((0, linked), (R.UNORIENTED, [True, False, True, True, True, True, False])):
        labels = check([(rows, curv)], dict(SMALL, normal_cos=cos, flags=flags))[3][0]
        assert [bool(labels[2 * k] == labels[2 * k + 1]) for k in range(len(linked))] == want
    assert linked == [True, False, True, False, True, False, False]
    _, _, counts, labels, _ = check([RC.curvature_threshold()], SMALL)
    assert list(counts[0]) == [1, 1, 1, 2] and list(labels[0]) == [0, 0, 0]
    # the distance: 0.25 away is near, nextafter(0.25) is not, to either side and in cells one and two away
    far = np.nextafter(np.float32(0.25), np.float32(1))
    pairs = []
    for frac in (0.0, 1.0 / 64, 5.0 / 64, 9.0 / 64, 13.0 / 64):
        for sign in (1.0, -1.0):
            for dist in (np.float32(0.25), far):
                a = np.array([frac, 2.0 * len(pairs), 0], np.float32)
                b = a.copy()
                b[0] = np.float32(a[0] + np.float32(sign) * dist)
                assert abs(float(b[0]) - float(a[0])) == float(dist)
                pairs.append((a, b, dist == np.float32(0.25)))
    rows = RC.rows6(np.array([q for a, b, _ in pairs for q in (a, b)]))
    _, _, counts, labels, _ = check([(rows, RC.smooth(rows.shape[0]))], dict(SMALL, tolerance=0.25))
    assert [bool(labels[0][2 * k] == labels[0][2 * k + 1]) for k in range(len(pairs))] == [bool(near) for _, _, near in pairs]
    curv = RC.smooth(rows.shape[0])
    curv[1::2] = RC.ROUGH            # the same with the second row of every pair a border row: attached iff near
    _, _, counts, labels, _ = check([(rows, curv)], dict(SMALL, tolerance=0.25))
    assert [bool(labels[0][2 * k + 1] >= 0) for k in range(len(pairs))] == [bool(near) for _, _, near in pairs] and counts[0, 3] == 10


def test_border_rules():
    rows, curv, want = RC.border_cases()
    _, info, counts, labels, _ = check([(rows, curv)], SMALL)
    np.testing.assert_array_equal(labels[0], want)
    assert list(counts[0]) == [8, 8, 8, 4]
    _, info, _, labels, _ = check([(rows[[2, 1, 0]], curv[[2, 1, 0]])], SMALL)
    assert list(labels[0]) == [0, 0, 1] and info[0, 0]["first_row"] == 1
    # a border row two cells from its smooth row (0.0197 apart at tolerance 0.02, cells 0 and 2), to either side
    for sign in (1.0, -1.0):
        pair = RC.rows6([[0.0055, 0, 1], [0.0055 + sign * 0.0197, 0, 1], [0.0, 0.0, 1.0 - 0.05]])
        for order in ([0, 1, 2], [1, 0, 2]):
            _, _, counts, labels, _ = check([(pair[order], np.array([0, RC.ROUGH, 0], np.float32))], dict(SMALL, tolerance=0.02))
            assert counts[0, 3] == 1 and labels[0][0] == labels[0][1] == 0
    # 5,000 identical rows, all border: one crowded cell and nothing to attach to
    same = np.tile(RC.rows6([[0.1, 0.2, 0.9]]), (5000, 1))
    _, _, counts, labels, _ = check([(same, np.full(5000, RC.ROUGH))], SMALL)
    assert list(counts[0]) == [0, 0, 0, 0] and (labels[0] == -1).all()
    curv = np.full(5000, RC.ROUGH)
    curv[[4000, 4999]] = 0           # two smooth rows among them, at the same place: every border row attaches to the first
    _, info, counts, _, _ = check([(same, curv)], SMALL)
    assert list(counts[0]) == [1, 1, 1, 4998] and info[0, 0]["n_rows"] == 5000 and info[0, 0]["first_row"] == 4000


def test_non_finite_values():
    rows, curv = RC.perpendicular_planes()
    rows[::97, 0] = np.nan
    rows[5::101, 1] = np.inf
    rows[7::103, 4] = np.nan
    rows[11::107, 5] = -np.inf
    curv[13::109] = np.nan
    curv[17::113] = np.inf
    _, info, counts, labels, _ = check([(rows, curv)], SMALL)
    with np.errstate(invalid="ignore"):
        border = np.isfinite(rows).all(axis=1) & ~(curv <= RC.THR)
    assert counts[0, 0] == 2 and counts[0, 3] == border.sum() > 15 and (labels[0][::97] == -1).all() and (labels[0][border] >= 0).all()
    rows[3, :3] = [1e30, -1e30, 1e30]            # eligible: it stretches the grid far past 1,024 cells
    with pytest.raises(_capi.PPFError):
        check([(rows, curv)], SMALL)
    rows[3, 3] = np.nan                          # the same row without a finite normal: out of the bounds
    check([(rows, curv)], SMALL)
    none = RC.rows6(np.zeros((300, 3)))
    none[:, 4] = np.nan
    assert list(check([(none, RC.smooth(300))], SMALL)[2][0]) == [0, 0, 0, 0]
    assert list(check([(RC.rows6(np.zeros((300, 3))), np.full(300, np.nan, np.float32))], SMALL)[2][0]) == [0, 0, 0, 0]


def test_unoriented_flag_and_perpendicular_planes():
    plane = RC.alternating_plane()
    _, info, counts, _, _ = check([plane], SMALL)
    assert list(counts[0]) == [2, 2, 2, 0] and list(info[0, :2]["n_rows"]) == [450, 450]
    _, info, counts, _, _ = check([plane], dict(SMALL, flags=R.UNORIENTED))
    assert list(counts[0]) == [1, 1, 1, 0] and info[0, 0]["n_rows"] == 900
    rows, curv = RC.perpendicular_planes()
    _, info, counts, _, _ = check([(rows, curv)], SMALL)
    assert list(counts[0]) == [2, 2, 2, 0] and list(info[0, :2]["n_rows"]) == [625, 600]
    assert cluster_clouds([upload(rows, curv)], dict(tolerance=0.01, min_size=1), return_info=True)[2][0, 2] == 1


def test_folded_chain():
    """10,000 rows 0.9 x tolerance apart in ten folded runs (test_gpu_clusters.chain), in shuffled row order and in chain order
    (the worst union paths).  The normal turns by 0.01 rad a step, far inside the 15 degrees, so the chain is one region though
    its ends' normals differ by a hundred radians; one step of 0.5 rad at row 6,000 cuts it in two."""
    from test_gpu_clusters import chain
    n, tol = 10000, 0.02
    xyz = chain(n, tol, fold=1000)
    for cut in (None, 6000):
        angle = 0.01 * np.arange(n) + (0.5 if cut else 0.0) * (np.arange(n) >= (cut or 0))
        rows = RC.rows6(xyz)
        rows[:, 3:] = np.stack([np.cos(angle), np.sin(angle), np.zeros(n)], axis=1)
        for order in (np.random.default_rng(n).permutation(n), np.arange(n)):
            _, info, counts, _, _ = check([(rows[order], RC.smooth(n))], dict(tolerance=tol))
            if cut:
                assert list(counts[0]) == [2, 2, 2, 0] and sorted(info[0, :2]["n_rows"]) == [n - cut, cut]
            else:
                assert list(counts[0]) == [1, 1, 1, 0] and info[0, 0]["n_rows"] == n


def blobs(sizes, seed=0, spread=0.002, pitch=0.2):
    rng = np.random.default_rng(seed)
    return RC.rows6(np.concatenate([rng.normal(size=(n, 3)) * spread + [pitch * i, 0.0, 1.0] for i, n in enumerate(sizes)]))


def test_ranking():
    rows = blobs([100, 100, 300, 100, 100, 100], seed=5)
    curv = RC.smooth(800)
    _, info, counts, _, _ = check([(rows, curv)], dict(min_size=100, max_size=200, max_regions=3))
    assert list(counts[0]) == [3, 5, 6, 0] and list(info[0]["first_row"]) == [0, 100, 500] and list(info[0]["n_rows"]) == [100] * 3
    _, info, counts, _, _ = check([(rows, curv)], dict(min_size=101))
    assert list(counts[0]) == [1, 1, 6, 0] and info[0, 0]["n_rows"] == 300
    # attached border rows count: the second blob's first row a border row makes its first_row 101 and leaves its size 100
    curv[100] = RC.ROUGH
    _, info, counts, _, _ = check([(rows, curv)], dict(min_size=100, max_size=200, max_regions=3))
    assert list(info[0]["first_row"]) == [0, 101, 500] and list(info[0]["n_rows"]) == [100] * 3 and counts[0, 3] == 1
    _, info, _, _, _ = check([(rows[::-1].copy(), RC.smooth(800))])
    assert list(info[0, :6]["n_rows"]) == [300, 100, 100, 100, 100, 100] and list(info[0, 1:6]["first_row"]) == [0, 100, 200, 600, 700]


def test_grid_limit():
    tol = 0.25
    h = tol * 0.5773
    fits = RC.rows6(np.array([[0, 0, 0], [0, 0, np.float32(1023.5 * h)]], np.float32))
    two = RC.smooth(2)
    _, _, counts, _, _ = check([(fits, two), (fits[:, [2, 0, 1, 3, 4, 5]], two)], dict(SMALL, tolerance=tol))
    assert list(counts[:, 2]) == [2, 2]
    over = RC.rows6(np.array([[0, 0, 0], [np.float32(1024.5 * h), 0, 0]], np.float32))
    with pytest.raises(_capi.PPFError) as e:
        region_clouds([upload(fits, two), upload(over, two)], dict(SMALL, tolerance=tol), return_info=True)
    assert e.value.status == _capi.PPF_ERR_INVALID and "ppf_prep_regions: in[1]" in str(e.value) and "1025 cells" in str(e.value)
    smallest = float(np.float32(str(e.value).rsplit(" ", 1)[1]))
    assert "smallest tolerance that fits" in str(e.value) and tol < smallest < tol * 1.002
    check([(over, two)], dict(SMALL, tolerance=smallest))
    with pytest.raises(_capi.PPFError):
        region_clouds([upload(over, two)], dict(SMALL, tolerance=float(np.nextafter(np.float32(smallest), np.float32(0)))))
    for bad in (dict(tolerance=0.0), dict(normal_cos=1.5), dict(curvature_threshold=-1.0), dict(min_size=0), dict(max_regions=257), dict(flags=2)):
        with pytest.raises(_capi.PPFError) as e:
            region_clouds([upload(fits, two)], bad)
        assert e.value.status == _capi.PPF_ERR_INVALID


FIVE = (0, 2, 65, 4097, 1500)


def test_clouds_in_one_call_equal_each_alone():
    clouds = [RC.patches(n, seed=50 + i) for i, n in enumerate(FIVE)]
    p = dict(tolerance=0.02, min_size=3, max_regions=40)
    found, info, counts, labels, _ = check(clouds, p)
    for i, (r, c) in enumerate(clouds):
        one, info1, counts1, labels1, _ = upload(r, c).regions(p, return_info=True, return_labels=True)
        assert info1.tobytes() == info[i].tobytes() and counts1.tobytes() == counts[i].tobytes() and labels1.tobytes() == labels[i].tobytes()
        for a, b in zip(one, found[i]):
            for x, y in zip(a.download(), b.download()):
                np.testing.assert_array_equal(bits(x), bits(y))
    assert counts[3, 0] == 40 and counts[4, 0] > 5
    last = found[4][1].download()
    del found[3], found[3][0]                     # the outputs share one block: the others outlive their siblings
    np.testing.assert_array_equal(bits(found[3][0].download()[0]), bits(last[0]))


def test_launch_and_sync_counts_do_not_depend_on_the_clouds():
    five = [RC.patches(n, seed=60 + i) for i, n in enumerate(FIVE)]
    for p in (dict(SMALL, tolerance=0.02), dict(min_size=5, max_size=9, max_regions=256, tolerance=0.03, normal_cos=0.5, flags=1,
                                                  curvature_threshold=np.inf)):
        s1 = check([five[3]], p)[4]
        s5 = check(five, p)[4]
        assert (s1["n_launches"], s1["n_host_syncs"]) == (s5["n_launches"], s5["n_host_syncs"]) == (LAUNCHES, 1)
    assert region_clouds([], return_info=True)[-1]["n_launches"] == 0
    empty = region_clouds([upload(*five[0])], return_info=True)[-1]
    assert (empty["n_launches"], empty["n_host_syncs"]) == (0, 0)
    # ppf_prep_clusters keeps its own count
    assert cluster_clouds([upload(*five[3])], return_info=True)[-1]["n_launches"] == LAUNCHES - 1


def test_repeated_and_concurrent_calls_give_the_same_bytes():
    cloud = upload(*RC.patches(6000, seed=70))
    p = dict(SMALL, tolerance=0.02, max_regions=100)

    def run():
        f, i, c, l, _ = cloud.regions(p, return_info=True, return_labels=True)
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
    rows = blobs([300, 200, 150], seed=8, pitch=0.3)
    rows[300:500, 2] -= np.float32(2.0)                  # the second blob lies behind the camera: z < 0, no pixel
    curv = RC.smooth(650)
    intr, size = (400.0, 400.0, 159.5, 119.5), (240, 320)
    _, info, _, _, _ = check([(rows, curv)], dict(min_size=10), intr=intr, image_size=size)
    assert info[0, 0]["box_xywh"][2] > 0 and not info[0, 1]["box_xywh"].any()
    assert info[0, 2]["box_xywh"][0] + info[0, 2]["box_xywh"][2] == 319      # u = 399 at its centre: clipped at the border
    _, info, _, _, _ = check([(rows, curv)], dict(min_size=10))
    assert not info["box_xywh"].any()
    K = np.array([[400.0, 0, 159.5], [0, 400.0, 119.5], [0, 0, 1]])
    _, info3, _, _ = region_clouds([upload(rows, curv)], dict(min_size=10), K, size, return_info=True)
    assert info3[0, 0]["box_xywh"].tolist() == R.regions(rows, dict(min_size=10), curv, intr=intr, image_size=size)[1][0]["box_xywh"].tolist()


def test_without_a_normal_or_curvature_condition_the_device_gives_its_clusters():
    rows, curv = RC.patches(5000, seed=80, degree=1.5)
    rows[::53, 0] = np.nan
    cloud = upload(rows, curv)
    for p in (dict(tolerance=0.02, min_size=1), dict(tolerance=0.025, min_size=4, max_size=60)):
        reg, rinfo, rcounts, rlabels, _ = cloud.regions(dict(p, max_regions=50, normal_cos=-1.0, curvature_threshold=np.inf),
                                                        return_info=True, return_labels=True)
        clu, cinfo, ccounts, clabels, _ = cloud.clusters(dict(p, max_clusters=50), return_info=True, return_labels=True)
        assert list(rcounts) == list(ccounts) + [0] and rinfo.tobytes() == cinfo.tobytes() and rlabels.tobytes() == clabels.tobytes()
        assert len(reg) == len(clu) > 20
        for a, b in zip(reg, clu):
            for x, y in zip(a.download(), b.download()):
                np.testing.assert_array_equal(bits(x), bits(y))


def test_rendered_frame_from_depth_to_regions(bottle):
    """from_depth(normals=...) -> regions on the rendered two-bottle frame, background and all: the figures of
    test_region_oracle.test_rendered_frame_with_its_background at tolerance 0.01, the oracle run on the device's own rows"""
    from test_gpu_frame import _render_frame
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    cloud = DeviceCloud.from_depth(depth, K, fp64=True, normals={})
    rows, curv = cloud.download()
    p = dict(tolerance=0.01)
    found, info, counts, labels, stats = cloud.regions(p, K, depth.shape, return_info=True, return_labels=True)
    assert_cloud(found, info, counts, labels, rows, curv, p, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), depth.shape)
    assert list(counts) == [8, 8, 71, 1081] and list(info["n_rows"][:8]) == [212390, 6461, 5551, 1526, 1228, 1134, 702, 113]
    assert (stats["n_launches"], stats["n_host_syncs"]) == (LAUNCHES, 1)
    cp = CloudProcessor(None, depth, [], [], [], 0.05, 0.05)
    cp.Deprojection(K, fp64=True, normals={})
    got = cp.ProposeRegions(K, p)
    assert cp.boxes == [tuple(int(v) for v in b) for b in info["box_xywh"][:8]] and [len(c) for c in got] == list(info["n_rows"][:8])
    assert cp.cluster_info.tobytes() == info[:8].tobytes()


def test_cpp_region_demo(tmp_path, bottle):
    from test_gpu_frame import _render_frame
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    exe = str(tmp_path / "region_demo")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "region_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    (tmp_path / "depth.f32").write_bytes(np.ascontiguousarray(depth, np.float32).tobytes())
    intr = [repr(float(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2])]
    r = subprocess.run([exe, str(tmp_path / "depth.f32"), str(depth.shape[0]), str(depth.shape[1])] + intr + ["0.01", "15", "0.03", "100"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cloud = DeviceCloud.from_depth(depth, K, fp64=True, normals={})
    cos = float(np.float32(np.cos(np.float32(15.0 / 180.0 * np.pi).astype(np.float64))))
    found, info, counts, labels, _ = cloud.regions(dict(tolerance=0.01, normal_cos=cos), K, depth.shape, return_info=True, return_labels=True)

    def checksum(c):
        rows, curv = c.download()
        return int(bits(rows).astype(np.uint64).sum() + bits(curv).astype(np.uint64).sum())
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"scene rows {len(cloud)} checksum {checksum(cloud)}"
    assert lines[1] == f"regions {counts[0]} valid {counts[1]} components {counts[2]} attached {counts[3]}"
    n = int(counts[0])
    assert n == 8
    for k in range(n):
        b = info[k]["box_xywh"]
        assert lines[2 + k] == (f"region {k}: rows {info[k]['n_rows']} first {info[k]['first_row']} box {b[0]} {b[1]} {b[2]} {b[3]} "
                                f"checksum {checksum(found[k])}")
    assert lines[2 + n] == f"launches {LAUNCHES} host_syncs 1"
    # the PCL-shaped surface: the same regions as index lists, ascending inside a region
    assert lines[3 + n] == f"pcl regions {n}"
    for k in range(n):
        idx = np.flatnonzero(labels == k)
        assert lines[4 + n + k] == f"pcl region {k}: size {idx.size} first {idx[0]} last {idx[-1]} sum {int(idx.sum())}"
