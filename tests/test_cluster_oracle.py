"""tests/cluster_oracle.py, the numpy / scipy restatement of ppf_prep_clusters that the device is held to byte for byte
(DESIGN.md §20), against things that do not depend on its k-d tree: an O(n^2) union by the same predicate on clouds of up to
2,000 rows, the rules of the specification on hand-made clouds, and two frames whose clusters were counted beforehand: the
rendered two-bottle frame and the reference's frame, each after plane_oracle.remove_planes."""
import os

import numpy as np
import pytest

import cluster_oracle as CL
import plane_oracle as P
import prep_data as D


def blobs(sizes, seed=0, spread=0.004, pitch=0.2):
    """one tight blob per size, far apart, rows in blob order"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(size=(n, 3)) * spread + [pitch * i, 0.0, 1.0] for i, n in enumerate(sizes)]).astype(np.float32)


@pytest.mark.parametrize("n,tol,seed", [(1, 0.1, 0), (2, 0.1, 1), (300, 0.05, 2), (1000, 0.06, 3), (2000, 0.05, 4), (2000, 0.08, 5)])
def test_components_against_the_quadratic_union(n, tol, seed):
    rng = np.random.default_rng(seed)
    cloud = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    cloud[rng.integers(0, n, n // 50)] = np.nan
    want = CL.brute_components(cloud, tol)
    np.testing.assert_array_equal(CL.components(cloud, tol), want)
    assert n < 300 or 3 < np.unique(want).size < n   # neither dust nor one lump


def test_the_predicate_is_closed_at_the_tolerance():
    tol = 0.25
    far = float(np.nextafter(np.float32(0.25), np.float32(1)))
    for axis in range(3):
        e = np.zeros(3, np.float32)
        e[axis] = 1
        cloud = np.stack([-far * e, 0 * e, tol * e]).astype(np.float32)   # 0 -- 0.25 linked, -0.25000003 -- 0 not
        assert list(CL.components(cloud, tol)) == [0, 1, 1]
        assert list(CL.brute_components(cloud, tol)) == [0, 1, 1]


def test_ranking_validity_and_truncation():
    cloud = blobs([100, 100, 300, 100, 50, 100, 100])
    found, info, counts, labels = CL.clusters(cloud, dict(min_size=60, max_size=200, max_clusters=3))
    assert list(counts) == [3, 5, 7]                                # the blob of 300 and the blob of 50 are not valid
    assert list(info["n_rows"]) == [100, 100, 100] and list(info["first_row"]) == [0, 100, 500]   # equal sizes: by first row
    assert (labels[:100] == 0).all() and (labels[100:200] == 1).all() and (labels[500:600] == 2).all()
    assert (labels[200:500] == -1).all() and (labels[600:] == -1).all()
    for r, (rows, curv) in enumerate(found):
        np.testing.assert_array_equal(rows[:, :3], cloud[labels == r])
    _, info, counts, _ = CL.clusters(cloud, dict(min_size=1))
    assert list(info["n_rows"][:7]) == [300, 100, 100, 100, 100, 100, 50] and list(counts) == [7, 7, 7]
    assert info[7].tobytes() == bytes(CL.INFO.itemsize)


def test_boxes_lo_hi_and_non_finite_rows():
    cloud = blobs([200, 150], seed=1)
    cloud[::17] = [np.nan, 0, 1]
    intr, size = (400.0, 400.0, 159.5, 119.5), (240, 320)
    found, info, counts, labels = CL.clusters(cloud, dict(min_size=10), intr=intr, image_size=size)
    assert (labels[::17] == -1).all() and list(counts) == [2, 2, 2]
    for r, (rows, _) in enumerate(found):
        assert np.isfinite(rows[:, :3]).all()
        np.testing.assert_array_equal(info[r]["lo"], rows[:, :3].min(axis=0))
        np.testing.assert_array_equal(info[r]["hi"], rows[:, :3].max(axis=0))
        u = np.floor(rows[:, 0].astype(np.float64) / rows[:, 2] * 400.0 + 159.5 + 0.5)
        assert info[r]["box_xywh"][0] == max(u.min(), 0) and info[r]["box_xywh"][0] + info[r]["box_xywh"][2] == min(u.max(), 319)
    assert info[1]["box_xywh"][0] + info[1]["box_xywh"][2] <= 319
    wide = CL.clusters(cloud * np.float32([10, 10, 1]), dict(min_size=10, tolerance=0.2), intr=intr, image_size=size)[1]
    assert wide[1]["box_xywh"][0] == 319 and wide[1]["box_xywh"][2] == 0   # the second blob projects to u = 959: clipped to the border
    assert not CL.clusters(cloud, dict(min_size=10))[1]["box_xywh"].any()                              # no intrinsics: zero


@pytest.fixture(scope="module")
def rendered():
    from test_gpu_frame import _render_frame
    scene, depth, boxes, K, objs, solid = _render_frame(np.load(os.path.join(D.GOLDEN, "bottle_model_xyzn.npy")))
    return P.remove_planes(scene)[0], depth, boxes, K


def test_rendered_frame_three_objects(rendered):
    """The plane-free rendered frame (18,010 rows) at the default tolerance 0.02: exactly its three objects, whose boxes are
    the boxes the frame was rendered with, one pixel larger each way (a rendered box excludes its last column and row)."""
    kept, depth, boxes, K = rendered
    assert kept.shape[0] == 18010
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    found, info, counts, labels = CL.clusters(kept, intr=intr, image_size=depth.shape)
    assert list(counts) == [3, 3, 3] and list(info["n_rows"][:3]) == [8317, 6553, 3140]
    assert [tuple(b) for b in info["box_xywh"][:3]] == [(72, 142, 143, 84), (275, 142, 107, 84), (446, 156, 76, 72)]
    assert sorted(tuple(b) for b in info["box_xywh"][:3]) == sorted((x, y, w + 1, h + 1) for x, y, w, h in boxes)
    assert (labels >= 0).all()
    # the nearest pair of rows to the tolerance is far from it in units of fp64 rounding: no rounding decides a link
    assert len(CL.clusters(kept, dict(tolerance=0.01, min_size=1, max_clusters=256))[0]) == 8
    assert CL.clusters(kept, dict(tolerance=0.005, min_size=1, max_clusters=256))[2][2] == 125


def test_reference_frame_after_two_planes():
    """The reference's frame after two planes (98,135 rows) at tolerance 0.01 and min_size 200: a dominant cluster of 68,320
    rows and 15 valid clusters, by the exact fp64 predicate (the same figures a k-d tree's own predicate gives)."""
    xyz, _, _, _ = D.c1_frame()
    kept = P.remove_planes(xyz, dict(n_hypotheses=256, max_planes=2))[0]
    assert kept.shape[0] == 98135
    found, info, counts, labels = CL.clusters(kept, dict(tolerance=0.01, min_size=200))
    assert info[0]["n_rows"] == 68320 and counts[0] == counts[1] == 15
    assert (info["n_rows"][:15] >= 200).all() and (np.diff(info["n_rows"][:15]) <= 0).all()
