"""tests/region_oracle.py, the numpy / scipy restatement of ppf_prep_regions that the device is held to byte for byte (DESIGN.md
§22), against things that do not depend on its k-d tree: the O(n^2) predicates on clouds of up to 2,000 rows, the rules of the
specification on hand-made clouds (tests/region_cases.py), cluster_oracle where the two specifications coincide, and two frames
whose regions were counted beforehand: the rendered two-bottle frame with its background, and the reference's frame after two
planes, whose 68,320-row cluster is what the stage was built for."""
import os

import numpy as np
import pytest

import cluster_oracle as CL
import depth_normals_oracle as O
import plane_oracle as P
import prep_data as D
import region_cases as RC
import region_oracle as R

SMALL = dict(min_size=1, max_regions=256)


def same(a, b):
    assert a[1].tobytes() == b[1].tobytes() and list(a[2]) == list(b[2])
    np.testing.assert_array_equal(a[3], b[3])
    assert len(a[0]) == len(b[0])
    for (r0, c0), (r1, c1) in zip(a[0], b[0]):
        assert r0.tobytes() == r1.tobytes() and c0.tobytes() == c1.tobytes()


@pytest.mark.parametrize("n,tol,cos,flags,seed", [(1, 0.1, 0.5, 0, 0), (2, 0.5, -1.0, 0, 1), (300, 0.1, 0.3, 0, 2), (1000, 0.08, 0.0, 1, 3),
                                                  (2000, 0.08, 0.3, 0, 4), (2000, 0.1, 0.7, 1, 5)])
def test_regions_against_the_quadratic_predicates(n, tol, cos, flags, seed):
    rows, curv = RC.random_cloud(n, seed)
    p = dict(SMALL, tolerance=tol, normal_cos=cos, flags=flags)
    got, want = R.regions(rows, p, curv), R.regions(rows, p, curv, brute=True)
    same(got, want)
    if n >= 300:
        assert 3 < want[2][2] < n and want[2][3] > 10 and want[1][0]["n_rows"] > 3   # neither dust nor one lump; borders attach


def test_agree_is_closed_at_normal_cos():
    rows, curv, cos, linked = RC.cosine_threshold()
    for brute in (False, True):
        labels = R.regions(rows, dict(SMALL, normal_cos=cos), curv, brute=brute)[3]
        assert [bool(labels[2 * k] == labels[2 * k + 1]) for k in range(len(linked))] == linked == [True, False, True, False, True, False, False]
        labels = R.regions(rows, dict(SMALL, normal_cos=cos, flags=R.UNORIENTED), curv, brute=brute)[3]
        assert [bool(labels[2 * k] == labels[2 * k + 1]) for k in range(len(linked))] == [True, False, True, True, True, True, False]
    # one step above: the pair whose dot product equals float32(0.8) no longer agrees
    above = float(np.nextafter(np.float32(cos), np.float32(1)))
    labels = R.regions(rows, dict(SMALL, normal_cos=above), curv)[3]
    assert labels[0] != labels[1] and labels[4] == labels[5]


def test_near_is_closed_at_the_tolerance():
    far = float(np.nextafter(np.float32(0.25), np.float32(1)))
    rows = RC.rows6([[-far, 0, 0], [0, 0, 0], [0.25, 0, 0]])
    for brute in (False, True):
        assert list(R.regions(rows, dict(SMALL, tolerance=0.25), brute=brute)[3]) == [1, 0, 0]


def test_smooth_is_closed_at_the_curvature_threshold():
    rows, curv = RC.curvature_threshold()
    smooth, border = R.kinds(rows, curv, RC.THR)
    assert list(smooth) == [True, False, False] and list(border) == [False, True, True]
    for brute in (False, True):
        _, info, counts, labels = R.regions(rows, SMALL, curv, brute=brute)
        assert list(counts) == [1, 1, 1, 2] and list(labels) == [0, 0, 0] and info[0]["n_rows"] == 3 and info[0]["first_row"] == 0
    # +inf: every eligible row of a comparable curvature is smooth; the NaN row still is not
    assert list(R.kinds(rows, curv, np.inf)[0]) == [True, True, False]


def test_border_rules():
    rows, curv, want = RC.border_cases()
    for brute in (False, True):
        found, info, counts, labels = R.regions(rows, SMALL, curv, brute=brute)
        np.testing.assert_array_equal(labels, want)
        assert list(counts) == [8, 8, 8, 4]
        assert list(info["n_rows"][:8]) == [2, 2, 2, 2, 1, 1, 1, 1] and list(info["first_row"][:8]) == [1, 3, 8, 10, 0, 4, 7, 13]
    # a region whose border row has the smaller index: first_row is still its smallest smooth row
    swapped = rows[[2, 1, 0]], curv[[2, 1, 0]]                 # border, its smooth row, the farther smooth row
    _, info, _, labels = R.regions(swapped[0], SMALL, swapped[1])
    assert list(labels) == [0, 0, 1] and info[0]["first_row"] == 1
    # all border: no region at all
    assert list(R.regions(rows, SMALL, np.full(14, RC.ROUGH))[2]) == [0, 0, 0, 0]


def test_non_eligible_rows():
    rows, curv = RC.perpendicular_planes()
    rows[5, 0], rows[6, 4], rows[7, 5], curv[8] = np.nan, np.inf, np.nan, np.nan
    _, info, counts, labels = R.regions(rows, SMALL, curv)
    assert list(labels[5:8]) == [-1, -1, -1] and labels[8] == 0 and list(counts) == [2, 2, 2, 1]
    assert list(info["n_rows"][:2]) == [622, 600]


@pytest.mark.parametrize("seed", [0, 1])
def test_without_a_normal_or_curvature_condition_the_regions_are_the_clusters(seed):
    rows, curv = RC.random_cloud(3000, seed, side=0.8, nan_share=0.0)
    rows[::41, :3] = np.nan
    for p in (dict(tolerance=0.05, min_size=1, max_size=0), dict(tolerance=0.06, min_size=3, max_size=40)):
        got = R.regions(rows, dict(p, max_regions=50, curvature_threshold=np.inf, normal_cos=-1.0), curv)
        want = CL.clusters(rows, dict(p, max_clusters=50), curv)
        assert list(got[2]) == list(want[2]) + [0]
        same((got[0], got[1], want[2], got[3]), want)
        assert want[2][0] > 5          # not one lump, not dust


def test_two_perpendicular_planes():
    rows, curv = RC.perpendicular_planes()
    assert list(CL.clusters(rows, dict(tolerance=0.01, min_size=1))[2]) == [1, 1, 1]
    _, info, counts, labels = R.regions(rows, SMALL, curv)
    assert list(counts) == [2, 2, 2, 0] and list(info["n_rows"][:2]) == [625, 600] and (labels[:625] == 0).all() and (labels[625:] == 1).all()


def test_unoriented():
    rows, curv = RC.alternating_plane()
    assert list(R.regions(rows, SMALL, curv)[1]["n_rows"][:3]) == [450, 450, 0]
    assert list(R.regions(rows, dict(SMALL, flags=R.UNORIENTED), curv)[1]["n_rows"][:2]) == [900, 0]


def test_ranking_validity_and_truncation():
    rng = np.random.default_rng(0)
    sizes = [100, 100, 300, 100, 50, 100, 100]
    xyz = np.concatenate([rng.normal(size=(n, 3)) * 0.002 + [0.2 * i, 0.0, 1.0] for i, n in enumerate(sizes)])
    rows, curv = RC.rows6(xyz), RC.smooth(sum(sizes))
    _, info, counts, labels = R.regions(rows, dict(min_size=60, max_size=200, max_regions=3), curv)
    assert list(counts) == [3, 5, 7, 0] and list(info["n_rows"]) == [100] * 3 and list(info["first_row"]) == [0, 100, 500]
    assert (labels[200:500] == -1).all() and (labels[600:] == -1).all()


@pytest.fixture(scope="module")
def rendered():
    from test_gpu_frame import _render_frame
    scene, depth, boxes, K, objs, solid = _render_frame(np.load(os.path.join(D.GOLDEN, "bottle_model_xyzn.npy")))
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    rows, curv = O.depth_normals(depth, intr, fp64=True)
    return rows, curv, depth, boxes, intr


def test_rendered_frame_with_its_background(rendered):
    """The rendered two-bottle frame as it comes from the depth image, background plane and all (230,400 rows, 12 without a
    normal, 2,024 border rows at the default curvature cut): no plane is removed.  At tolerance 0.02 the background is region
    0 and each bottle one region, whose box is the cluster's box of test_cluster_oracle less, for the second, one column of
    silhouette pixels that attach to nothing; the solid falls into three regions."""
    rows, curv, depth, boxes, intr = rendered
    assert rows.shape[0] == 230400 and int(np.isnan(curv).sum()) == 12 and int((curv > RC.THR).sum()) == 2024
    found, info, counts, labels = R.regions(rows, dict(tolerance=0.02), curv, intr, depth.shape)
    assert list(counts) == [6, 6, 45, 1264]
    assert list(info["n_rows"][:6]) == [212390, 8108, 6355, 1233, 1190, 140]
    assert [tuple(b) for b in info["box_xywh"][1:3]] == [(72, 142, 143, 84), (276, 142, 106, 84)]
    assert int((labels < 0).sum()) == 984
    _, info, counts, _ = R.regions(rows, dict(tolerance=0.01), curv, intr, depth.shape)
    assert list(counts) == [8, 8, 71, 1081] and list(info["n_rows"][:8]) == [212390, 6461, 5551, 1526, 1228, 1134, 702, 113]


def test_reference_frame_after_two_planes():
    """The reference's frame after two planes (98,135 rows; 93,477 smooth, 4,646 border, 12 without a normal) at tolerance 0.01
    and min_size 200, where Euclidean clustering leaves one cluster of 68,320 rows.  With the default 15 degrees and curvature
    cut 0.03 that cluster does NOT divide: 67,166 of its rows are one region, 1,154 in none -- normals from a 7 x 7 window turn
    gradually where two surfaces touch.  At 5 degrees (normal_cos 0.9961947) and curvature cut 0.01 it divides into nine valid
    regions of 26,101, 9,987, 5,864, 5,327, 4,949, 1,816, 540, 366 and 284 rows, 13,086 rows in none."""
    xyz, depth, _, intr = D.c1_frame()
    rows, curv = O.depth_normals(depth, intr, fp64=True)
    assert rows[:, :3].tobytes() == xyz.tobytes()
    kept, kcurv, _, _ = P.remove_planes(rows, dict(n_hypotheses=256, max_planes=2), curv)
    assert kept.shape[0] == 98135
    smooth, border = R.kinds(kept, kcurv, RC.THR)
    assert (int(smooth.sum()), int(border.sum())) == (93477, 4646)
    blob = CL.clusters(kept[:, :3], dict(tolerance=0.01, min_size=200))[3] == 0
    assert int(blob.sum()) == 68320
    _, info, counts, labels = R.regions(kept, dict(tolerance=0.01, min_size=200), kcurv)
    assert list(counts) == [15, 15, 153, 3782]
    assert list(info["n_rows"][:15]) == [67166, 8353, 4308, 4289, 3865, 2657, 2278, 908, 637, 386, 304, 279, 274, 254, 218]
    inside = dict(zip(*np.unique(labels[blob], return_counts=True)))
    assert inside == {-1: 1154, 0: 67166}
    _, info, counts, labels = R.regions(kept, dict(tolerance=0.01, min_size=200, normal_cos=0.9961947, curvature_threshold=0.01), kcurv)
    assert list(counts) == [21, 21, 464, 10374]
    inside = np.unique(labels[blob], return_counts=True)[1]
    assert sorted(inside.tolist(), reverse=True) == [26101, 13086, 9987, 5864, 5327, 4949, 1816, 540, 366, 284]
