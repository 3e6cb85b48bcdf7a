"""The numpy oracle of ppf_depth_edges (tests/depth_edges_oracle.py) held to the specification of DESIGN.md §35: its two
implementations against each other on seeded images with every kind of invalid value, at the closure of the jump threshold, on
images whose answer is known (a sphere alone and over a wall, a step, a sensor's holes), against ppf_depth_segments' step, and
on the fact the stage was proposed with: the curvature of depth normals marks no silhouette pixel."""
import numpy as np
import pytest

import depth_edges_oracle as E
import depth_motion_cases as M
import depth_normals_oracle as N
import depth_segments_oracle as S
import depth_volume_cases as V
from test_depth_filter_oracle import seeded, step_image

ONE = np.float32(1.0)


def bit(mask, b):
    return (mask & b) != 0


def seeded_normals(rng, depth, nan_share=0.05, curved_share=0.2, **depth_kw):
    """a normals cloud for the kept pixels of `depth`: unit normals, some rows NaN, some curvatures above 0.03, some NaN"""
    kept = N.keep_mask(N.metric_depth(depth, depth_kw.get("depth_scale", 0.001)), depth_kw.get("z_min", 0.0), depth_kw.get("z_max", 0.0))
    n = int(kept.sum())
    rows = rng.normal(size=(n, 6)).astype(np.float32)
    rows[:, 3:6] /= np.linalg.norm(rows[:, 3:6], axis=1, keepdims=True)
    curv = (0.03 * rng.random(n)).astype(np.float32)
    curv[rng.random(n) < curved_share] = np.float32(0.2)
    bad = rng.random(n) < nan_share
    rows[bad, 3 + rng.integers(0, 3, size=int(bad.sum()))] = np.nan
    curv[rng.random(n) < 0.03] = np.nan
    return rows, curv


@pytest.mark.parametrize("max_gap", range(0, 9))
def test_the_two_implementations_agree_at_every_max_gap_in_both_formats(max_gap):
    rng = np.random.default_rng(300 + max_gap)
    for dtype, kw in ((np.float32, {}), (np.uint16, dict(depth_scale=0.001))):
        for density in (0.85, 0.4):
            img = seeded(rng, (13, 23), density=density, dtype=dtype)
            got, want = E.edges(img, max_gap=max_gap, **kw), E.edges_loops(img, max_gap=max_gap, **kw)
            assert E.same(got, want), (max_gap, dtype, got[2], want[2])
            st = got[2]
            assert st["n_kept"] == int(N.keep_mask(N.metric_depth(img)).sum()) and st["n_edge"] <= st["n_kept"]
            assert not got[0][~N.keep_mask(N.metric_depth(img))].any()
            assert st["n_occluding"] > 0 and st["n_occluded"] > 0 and st["n_boundary"] > 0


def test_quad_term_cuts_normals_selections_and_clouds_equal_the_pixel_loops():
    rng = np.random.default_rng(320)
    img = seeded(rng, (14, 21))
    intr = (40.0, 41.0, 10.2, 6.7)
    nrm = seeded_normals(rng, img)
    cut = dict(z_min=1.0, z_max=1.3)
    for kw in (dict(depth_quad=0.01), dict(depth_quad=0.02, depth_abs=0.0), dict(cut), dict(intr=intr), dict(intr=intr, fp64=True),
               dict(normals=nrm), dict(normals=nrm, select=E.CURVATURE), dict(normals=nrm, curvature_threshold=np.inf, max_gap=4),
               dict(normals=seeded_normals(rng, img, **cut), select=E.OCCLUDED | E.BOUNDARY, **cut), dict(intr=intr, select=E.OCCLUDED)):
        kw = dict(kw)
        it = kw.pop("intr", None)
        got = E.edges(img, it, **kw)
        assert E.same(got, E.edges_loops(img, it, **kw)), kw
        if got[1] is not None:
            assert got[2]["n_rows"] == got[2]["n_selected"] - got[2]["n_no_normal"] == got[1][0].shape[0] > 0
    got = E.edges(img, normals=nrm)
    assert got[2]["n_no_normal"] > 0 and got[2]["n_curvature"] > 0
    assert not bit(E.edges(img, normals=nrm, curvature_threshold=np.inf)[0], E.CURVATURE).any()


def test_jump_threshold_closure():
    """fabs(dZ) == depth_abs is no edge, one ulp further is OCCLUDING on the near pixel and OCCLUDED on the far one: zp 1.0,
    zq 1.0078125 and depth_abs 0.0078125 are exact in float32"""
    zq = np.float32(1.0078125)
    for q, edge in ((zq, False), (np.nextafter(zq, np.float32(2)), True)):
        img = np.array([[ONE, q]], np.float32)
        got = E.edges(img, depth_abs=0.0078125)
        assert E.same(got, E.edges_loops(img, depth_abs=0.0078125))
        assert got[0].tolist() == ([[E.OCCLUDING, E.OCCLUDED]] if edge else [[0, 0]])
    # the quad term: 0.0078125 = 0.0078125 / 1.0078125 * (1.0 * 1.0078125) only up to rounding, so state it through the rule
    dq = np.float32(0.0077)
    thr = np.float64(dq) * (np.float64(ONE) * np.float64(zq))
    img = np.array([[ONE], [zq]], np.float32)
    assert E.edges(img, depth_abs=0.0, depth_quad=dq)[0].tolist() == ([[E.OCCLUDING], [E.OCCLUDED]] if np.float64(zq) - 1.0 > thr else [[0], [0]])
    assert E.edges(img, depth_abs=0.0, depth_quad=0.0)[0].tolist() == [[E.OCCLUDING], [E.OCCLUDED]]
    assert not E.edges(np.full((3, 3), ONE), depth_abs=0.0)[0].any()          # equal depths never jump


def sphere():
    img = V.render_sphere(np.eye(4))
    on = N.keep_mask(img)
    H, W = on.shape
    pad = np.pad(on, 1, constant_values=True)      # the image border is no neighbour
    rim = np.zeros_like(on)
    for dv, du in E.DIRECTIONS:
        rim |= on & ~pad[1 + dv:1 + dv + H, 1 + du:1 + du + W]
    return img, on, rim


def test_a_sphere_alone_has_its_rim_as_boundary():
    img, on, rim = sphere()
    assert img.shape == (120, 160) and int(on.sum()) == 1476 and int(rim.sum()) == 172
    mask, _, st = E.edges(img, max_gap=2)
    assert np.array_equal(bit(mask, E.BOUNDARY), rim) and st["n_boundary"] == 172
    assert E.same(E.edges(img), E.edges_loops(img))


@pytest.mark.parametrize("depth_abs,inside", [(0.02, 32), (0.01, 220), (0.005, 608)])
def test_a_sphere_over_a_wall(depth_abs, inside):
    """every rim pixel is OCCLUDING (the jump is >= 0.2 m), nothing off the sphere is, the wall is only ever OCCLUDED, and
    nothing is BOUNDARY; the grazing rim of 4.7 mm pixels adds OCCLUDING pixels inside the sphere, fewest at the default"""
    img, on, rim = sphere()
    img = img.copy()
    img[~on] = ONE
    mask, _, st = E.edges(img, depth_abs=depth_abs)
    occ = bit(mask, E.OCCLUDING)
    assert (occ & rim).sum() == 172 and not (occ & ~on).any()
    assert set(np.unique(mask[~on]).tolist()) == {0, E.OCCLUDED}
    assert st["n_boundary"] == 0 and not bit(mask, E.BOUNDARY).any()
    assert int((occ & on & ~rim).sum()) == inside and st["n_occluding"] == 172 + inside
    if depth_abs == 0.02:
        assert E.same(E.edges(img), E.edges_loops(img))


def test_a_step_is_its_two_columns_and_the_image_border_is_no_edge():
    mask, _, st = E.edges(step_image())
    want = np.zeros((12, 16), np.uint8)
    want[:, 7], want[:, 8] = E.OCCLUDING, E.OCCLUDED
    assert np.array_equal(mask, want)
    assert st["n_occluding"] == st["n_occluded"] == 12 and st["n_boundary"] == 0 and st["n_edge"] == 24
    for gap in (0, 8):
        assert np.array_equal(E.edges(step_image(), max_gap=gap)[0], want)
    assert not E.edges(np.full((5, 7), ONE))[0].any() and not E.edges(np.full((1, 1), ONE))[0].any()


def test_max_gap_0_marks_every_kept_pixel_beside_a_hole():
    img = np.full((7, 9), ONE)
    img[3, 4] = 0
    img[0, 0] = np.nan
    mask = E.edges(img, max_gap=0)[0]
    want = np.zeros((7, 9), np.uint8)
    want[2:5, 3:6] = E.BOUNDARY
    want[0:2, 0:2] = E.BOUNDARY
    want[3, 4] = want[0, 0] = 0
    assert np.array_equal(mask, want)
    # one pixel wide with the same surface behind it: a hole, not an edge; the walks across the corner hole leave the image
    wider = E.edges(img, max_gap=1)[0]
    want[:] = 0
    want[0, 1] = want[1, 0] = want[1, 1] = E.BOUNDARY
    assert np.array_equal(wider, want)


def test_a_gap_that_runs_into_the_image_border_is_a_boundary():
    img = np.full((3, 8), ONE)
    img[:, 5:] = 0
    for gap in (0, 2, 3, 8):
        mask = E.edges(img, max_gap=gap)[0]
        assert mask[:, 4].tolist() == [E.BOUNDARY] * 3 and not mask[:, :4].any(), gap
        assert E.same(E.edges(img, max_gap=gap), E.edges_loops(img, max_gap=gap))


def test_a_sensors_holes_stop_being_boundaries_at_max_gap_2():
    img = M.sensor(M.render(np.eye(4)), 3)
    assert img.dtype == np.float32 and int((~N.keep_mask(img)).sum()) == 988
    got = {gap: E.edges(img, max_gap=gap)[2] for gap in (0, 1, 2)}
    assert [got[g]["n_boundary"] for g in (0, 1, 2)] == [6218, 441, 92]
    assert [got[g]["n_occluding"] for g in (0, 1, 2)] == [413, 469, 474]
    assert [got[g]["n_occluded"] for g in (0, 1, 2)] == [426, 486, 492]
    assert got[2]["n_boundary"] < 0.05 * got[0]["n_boundary"]
    assert got[2]["n_kept"] == 120 * 160 - 988


def test_jump_is_the_negation_of_the_segments_step():
    """for 4-adjacent kept pairs at equal thresholds: the segments oracle links two kept pixels without normals iff step,
    so on an image of exactly two kept pixels they share a segment iff the edge oracle marks neither"""
    rng = np.random.default_rng(330)
    for _ in range(60):
        zp = np.float32(0.5 + rng.random())
        zq = np.float32(zp + rng.choice([-1, 1]) * rng.choice([0.0049, 0.005, 0.0051, 0.02, 0.0]) * (1 + 0.001 * rng.normal()))
        da, dq = float(rng.choice([0.005, 0.0, 0.02])), float(rng.choice([0.0, 0.004]))
        for img in (np.array([[zp, zq]], np.float32), np.array([[zp], [zq]], np.float32)):
            mask = E.edges(img, depth_abs=da, depth_quad=dq)[0]
            labels = S.segments(img, depth_abs=da, depth_quad=dq, min_size=2)[0]
            linked = bool((labels == 0).all())
            assert linked == (not mask.any()), (zp, zq, da, dq)
            assert bool(E.jump(np.float64(zp), np.float64(zq), da, dq)) == (not linked)


def test_curvature_of_depth_normals_marks_no_silhouette_and_the_default_selection_holds_all_of_it():
    """the clean analytic scene with default normals: 124 pixels have curvature > 0.03 and none of the 452 OCCLUDING pixels is
    among them; the default select takes every OCCLUDING pixel, and the cloud leaves out only those without a normal"""
    img = M.render(np.eye(4)).astype(np.float32)
    intr = M.intrinsics()
    nrm = N.depth_normals(img, intr)
    mask, cloud, st = E.edges(img, normals=nrm)
    occ, cur = bit(mask, E.OCCLUDING), bit(mask, E.CURVATURE)
    assert (int(cur.sum()), int(occ.sum()), int((occ & cur).sum())) == (124, 452, 0)
    only, cloud_c, st_c = E.edges(img, normals=nrm, select=E.CURVATURE)
    assert st_c["n_selected"] == st_c["n_rows"] == 124 and not (bit(only, E.CURVATURE) & occ).any()
    sel = (mask & E.DEFAULTS["select"]) != 0
    assert (sel & occ).sum() == 452 and st["n_selected"] == 576 and st["n_no_normal"] == 3 and st["n_rows"] == 573
    index = np.full(mask.shape, -1)
    index[N.keep_mask(img)] = np.arange(nrm[0].shape[0])
    take = index[sel]
    take = take[np.isfinite(nrm[0][take, 3:6]).all(axis=1)]
    assert cloud[0].tobytes() == nrm[0][take].tobytes() and cloud[1].tobytes() == nrm[1][take].tobytes()


def test_parameter_ranges_and_a_wrong_row_count():
    img = np.full((4, 6), ONE)
    for kw in (dict(depth_abs=-1.0), dict(depth_abs=np.nan), dict(depth_quad=np.inf), dict(max_gap=-1), dict(max_gap=9),
               dict(curvature_threshold=-0.1), dict(curvature_threshold=np.nan), dict(select=0), dict(select=16), dict(flags=1)):
        with pytest.raises(ValueError):
            E.edges(img, **kw)
        with pytest.raises(ValueError):
            E.edges_loops(img, **kw)
    with pytest.raises(ValueError):
        E.edges(img, normals=(np.zeros((3, 6), np.float32), np.zeros(3, np.float32)))
