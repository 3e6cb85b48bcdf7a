"""The numpy oracle of ppf_depth_segments (tests/depth_segments_oracle.py) held to the specification of DESIGN.md §24: its two
implementations against each other on seeded images, images whose answer is known in closed form (a constant, the three
threshold closures, a chessboard, the border rule's two tie-breaks, the ranking's, the size bounds) and the window of the
reference's own frame whose counts the stage was proposed with."""
import numpy as np
import pytest

import depth_filter_oracle as F
import depth_normals_oracle as N
import depth_segments_oracle as S
import prep_data as D
from test_depth_filter_oracle import seeded

ONE = np.float32(1.0)


def seeded_normals(rng, depth, nan_share=0.05, border_share=0.2, **depth_kw):
    """a normals cloud for the image's kept pixels: unit normals of two families that disagree at the default normal_cos,
    tilted a little inside a family, some NaN; curvature below, above and exactly at 0.03, some NaN"""
    z = N.metric_depth(depth, depth_kw.get("depth_scale", 0.001))
    kept = N.keep_mask(z, depth_kw.get("z_min", 0.0), depth_kw.get("z_max", 0.0))
    vs, us = np.nonzero(kept)
    n = len(vs)
    base = np.where(((us // 23 + vs // 11) % 2 == 0)[:, None], np.array([0.0, 0.0, -1.0]), np.array([0.6, 0.0, -0.8]))
    nrm = base + 0.08 * rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    sign = np.where(rng.random(n) < 0.1, -1.0, 1.0)[:, None]       # a few flipped: only |dot| agrees
    rows = np.zeros((n, 6), np.float32)
    rows[:, 3:6] = (nrm * sign).astype(np.float32)
    rows[rng.random(n) < nan_share, 3 + rng.integers(0, 3)] = np.nan
    curv = (0.02 * rng.random(n)).astype(np.float32)
    hot = rng.random(n) < border_share
    curv[hot] = np.float32(0.03) + (0.05 * rng.random(int(hot.sum()))).astype(np.float32)
    curv[rng.random(n) < 0.02] = np.float32(0.03)
    curv[rng.random(n) < 0.02] = np.nan
    return rows, curv


@pytest.mark.parametrize("flags", [0, S.EIGHT, S.UNORIENTED, S.EIGHT | S.UNORIENTED])
def test_the_two_implementations_agree_on_seeded_images(flags):
    rng = np.random.default_rng(240 + flags)
    for shape, dtype in (((23, 41), np.float32), ((17, 70), np.uint16), ((1, 9), np.float32), ((9, 1), np.float32)):
        img = seeded(rng, shape, dtype=dtype)
        for kw in (dict(min_size=1), dict(min_size=3, max_size=40, max_segments=5, depth_abs=0.003, depth_quad=0.002)):
            assert S.same(S.segments(img, flags=flags, **kw), S.segments_bfs(img, flags=flags, **kw)), (shape, kw)
            nrm = seeded_normals(rng, img)
            a, b = S.segments(img, normals=nrm, flags=flags, **kw), S.segments_bfs(img, normals=nrm, flags=flags, **kw)
            assert S.same(a, b), (shape, kw)
            if shape == (23, 41):
                assert a[3]["n_attached"] > 0 and a[3]["n_eligible"] < a[3]["n_kept"] and a[2][2] > 1


def test_a_constant_image_is_one_segment():
    img = np.full((20, 30), np.float32(0.8125))
    labels, info, counts, stats = S.segments(img)
    assert counts == (1, 1, 1) and not labels.any() and stats == dict(n_kept=600, n_eligible=600, n_smooth=600, n_attached=0)
    assert info == [dict(n_pixels=600, n_border=0, first_pixel=0, box_xywh=(0, 0, 29, 19), z_lo=np.float32(0.8125), z_hi=np.float32(0.8125))]


def plateaus(zq):
    img = np.full((4, 6), ONE)
    img[:, 3:] = zq
    return img


def test_depth_threshold_closure():
    zq = np.float32(1.0078125)                    # 1 + 2^-7: the step is depth_abs exactly
    for q, linked in ((zq, True), (np.nextafter(zq, np.float32(2)), False)):
        for flags in (0, S.EIGHT):
            _, _, counts, _ = S.segments(plateaus(q), depth_abs=0.0078125, min_size=1, flags=flags)
            assert counts[2] == (1 if linked else 2)
    # the quad term alone: Zp * Zq = 2 and the step is 1, so depth_quad 0.5 is the closure
    for q, linked in ((np.float32(0.5), True), (np.nextafter(np.float32(0.5), np.float32(0)), False)):
        assert S.segments(plateaus(np.float32(2.0)), depth_abs=0.0, depth_quad=q, min_size=1)[2][2] == (1 if linked else 2)


def with_normals(img, nrm_of, curv_of):
    vs, us = np.nonzero(N.keep_mask(img))
    rows = np.zeros((len(vs), 6), np.float32)
    rows[:, 3:6] = [nrm_of(v, u) for v, u in zip(vs, us)]
    return rows, np.array([curv_of(v, u) for v, u in zip(vs, us)], np.float32)


def test_normal_cos_closure():
    c = np.float32(0.5)
    for q, linked in ((c, True), (np.nextafter(c, np.float32(0)), False)):
        # normals are taken as they are: across the edge the dot is q exactly, inside the right half 1 + q * q
        nrm = with_normals(np.full((4, 6), ONE), lambda v, u: (0, 0, 1) if u < 3 else (1, 0, q), lambda v, u: 0.0)
        counts = S.segments(np.full((4, 6), ONE), normals=nrm, normal_cos=0.5, min_size=1)[2]
        assert counts[2] == (1 if linked else 2)
    # a flipped normal agrees only on |dot|
    nrm = with_normals(np.full((4, 6), ONE), lambda v, u: (0, 0, 1) if u < 3 else (0, 0, -1), lambda v, u: 0.0)
    assert S.segments(np.full((4, 6), ONE), normals=nrm, min_size=1)[2][2] == 2
    assert S.segments(np.full((4, 6), ONE), normals=nrm, min_size=1, flags=S.UNORIENTED)[2][2] == 1


def test_curvature_threshold_closure():
    t = np.float32(0.03)
    img = np.full((3, 5), ONE)
    for cv, smooth in ((t, True), (np.nextafter(t, ONE), False), (np.float32(np.nan), False)):
        nrm = with_normals(img, lambda v, u: (0, 0, 1), lambda v, u: cv if (v, u) == (1, 2) else 0.0)
        _, info, counts, stats = S.segments(img, normals=nrm, min_size=1)
        assert stats["n_smooth"] == (15 if smooth else 14) and stats["n_attached"] == (0 if smooth else 1)
        assert counts == (1, 1, 1) and info[0]["n_pixels"] == 15 and info[0]["n_border"] == (0 if smooth else 1)
    nrm = with_normals(img, lambda v, u: (0, 0, 1), lambda v, u: 7.0)
    assert S.segments(img, normals=nrm, min_size=1, curvature_threshold=np.inf)[3]["n_smooth"] == 15
    assert S.segments(img, normals=nrm, min_size=1)[2] == (0, 0, 0)            # all border, nothing to attach to


def chessboard(shape):
    v, u = np.mgrid[0:shape[0], 0:shape[1]]
    return np.where((u + v) % 2 == 0, ONE, np.float32(0)).astype(np.float32)


def test_chessboard_under_both_connectivities():
    img = chessboard((7, 9))
    kept = int((img > 0).sum())
    labels, _, counts, _ = S.segments(img, min_size=1, max_segments=256)
    assert counts == (kept, kept, kept) and sorted(labels[img > 0]) == list(range(kept))
    labels, info, counts, _ = S.segments(img, min_size=1, flags=S.EIGHT)
    assert counts == (1, 1, 1) and info[0]["n_pixels"] == kept and (labels[img > 0] == 0).all() and (labels[img == 0] == -1).all()


def test_border_tie_goes_to_the_smaller_pixel_index():
    """a border pixel between two smooth pixels equally far in Z that do not link each other: the left one (smaller index)"""
    img = np.array([[0.99, 1.0, 1.01]], np.float32)
    img[0, 0], img[0, 2] = np.float32(1.0) - np.float32(2.0 ** -7), np.float32(1.0) + np.float32(2.0 ** -7)
    nrm = with_normals(img, lambda v, u: (0, 0, 1), lambda v, u: 1.0 if u == 1 else 0.0)
    labels, info, counts, stats = S.segments(img, normals=nrm, depth_abs=0.0078125, min_size=1)
    assert counts == (2, 2, 2) and stats["n_attached"] == 1
    assert labels.tolist() == [[0, 0, 1]] and info[0]["first_pixel"] == 0 and info[0]["n_border"] == 1 and info[0]["box_xywh"] == (0, 0, 1, 0)
    # vertically the upper neighbour is the smaller index
    labels = S.segments(np.ascontiguousarray(img.T), normals=nrm, depth_abs=0.0078125, min_size=1)[0]
    assert labels.tolist() == [[0], [0], [1]]


def test_border_pixel_goes_to_the_nearer_in_z():
    img = np.array([[1.0, 1.004, 1.006]], np.float32)
    nrm = with_normals(img, lambda v, u: (0, 0, 1), lambda v, u: 1.0 if u == 1 else 0.0)
    labels, info, _, _ = S.segments(img, normals=nrm, depth_abs=0.005, min_size=1)
    assert labels.tolist() == [[1, 0, 0]] and info[0]["first_pixel"] == 2 and info[0]["z_lo"] == img[0, 1]
    # out of step with both: it joins nothing
    img[0, 1] = 1.5
    labels, _, counts, stats = S.segments(img, normals=nrm, depth_abs=0.005, min_size=1)
    assert labels.tolist() == [[0, -1, 1]] and stats["n_attached"] == 0 and counts == (2, 2, 2)


def test_ranking_ties_go_by_first_pixel_and_the_size_bounds():
    img = np.zeros((5, 12), np.float32)
    img[0:2, 0:3] = 1.0        # 6 pixels, first pixel 0
    img[3:5, 0:3] = 1.0        # 6 pixels, first pixel 36
    img[0:4, 5:9] = 1.0        # 16 pixels
    img[4, 11] = 1.0           # 1 pixel
    labels, info, counts, _ = S.segments(img, min_size=1)
    assert counts == (4, 4, 4) and [(i["n_pixels"], i["first_pixel"]) for i in info] == [(16, 5), (6, 0), (6, 36), (1, 59)]
    assert labels[0, 0] == 1 and labels[3, 0] == 2 and labels[0, 5] == 0 and labels[4, 11] == 3
    assert S.segments(img, min_size=6)[2] == (3, 3, 4) and S.segments(img, min_size=7)[2] == (1, 1, 4)
    labels, info, counts, _ = S.segments(img, min_size=1, max_size=6)
    assert counts == (3, 3, 4) and [i["first_pixel"] for i in info] == [0, 36, 59] and labels[0, 5] == -1
    labels, info, counts, _ = S.segments(img, min_size=1, max_segments=2)
    assert counts == (2, 4, 4) and len(info) == 2 and labels[3, 0] == -1 and labels[4, 11] == -1


def test_parameter_ranges():
    img = np.full((2, 2), ONE)
    for kw in (dict(depth_abs=-1.0), dict(depth_abs=np.nan), dict(depth_quad=np.inf), dict(normal_cos=1.5), dict(curvature_threshold=np.nan),
               dict(min_size=0), dict(max_size=-1), dict(max_segments=0), dict(max_segments=257), dict(flags=4)):
        with pytest.raises(ValueError):
            S.segments(img, **kw)
    with pytest.raises(ValueError):
        S.segments(img, normals=(np.zeros((3, 6), np.float32), np.zeros(3, np.float32)))


def reference_window():
    """the 160 x 224 window of the reference frame that tests/test_gpu_depth_filter.py cuts, filtered, with its depth normals"""
    _, depth, box, intr = D.c1_frame()
    x, y, w, h = box
    r0 = int(np.clip(y + h // 2 - 80, 0, depth.shape[0] - 160))
    c0 = int(np.clip(x + w // 2 - 112, 0, depth.shape[1] - 224))
    win = np.ascontiguousarray(depth[r0:r0 + 160, c0:c0 + 224])
    shifted = (intr[0], intr[1], intr[2] - c0, intr[3] - r0)
    filtered = F.filter_depth(win)[0]
    return win, filtered, shifted, N.depth_normals(filtered, shifted, fp64=True)


@pytest.fixture(scope="module")
def window():
    return reference_window()


def test_reference_window_counts(window):
    """The stage does something on real data: both implementations give 37 components on the window, 7 of them valid (the
    largest 26,282 of the 29,575 kept pixels, 306 border pixels attached), 20 components under 8-connectivity and 32 on depth
    alone.  (The proposal quoted 171 / 12 / 19,924, 66 and 157 from a prototype; no reading of the specification -- raw or
    filtered window, the window's or the frame's normals, either back-projection -- gives those, and the two
    implementations here agree with each other, so the counts pinned are theirs.)"""
    _, filtered, _, nrm = window
    got = S.segments(filtered, normals=nrm)
    _, info, counts, stats = got
    assert counts == (7, 7, 37) and info[0]["n_pixels"] == 26282
    assert counts[0] >= 2
    assert stats == dict(n_kept=29575, n_eligible=29575, n_smooth=29091, n_attached=306) and stats["n_kept"] == nrm[0].shape[0]
    assert S.segments(filtered, normals=nrm, flags=S.EIGHT)[2] == (7, 7, 20)
    assert S.segments(filtered)[2] == (7, 7, 32)
    assert S.same(got, S.segments_bfs(filtered, normals=nrm))
