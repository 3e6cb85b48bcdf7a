"""The numpy oracle of ppf_depth_filter (tests/depth_filter_oracle.py) held to the specification of DESIGN.md §23: against
a per-pixel restatement in Python doubles on seeded images with every kind of invalid value, at the two threshold closures,
on images whose answer is known in closed form (a constant, a step, a lone pixel, radius 0) and on the reference's own frame,
whose counts and downstream figures are the ones the stage was proposed with."""
import numpy as np
import pytest

import depth_filter_oracle as F
import depth_normals_oracle as N
import prep_data as D

BAD = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -0.5, -1e-30], np.float32)


def seeded(rng, shape, density=0.85, dtype=np.float32):
    """a smooth surface whose slope and noise stay inside the default thresholds, depth steps far above them, and holes of
    every invalid kind: most pixels are supported, those around a hole or on a step are not"""
    rows, cols = shape
    v, u = np.mgrid[0:rows, 0:cols]
    z = 1.0 + 0.05 * np.sin(u / 15.0) + 0.04 * np.cos(v / 9.0) + 0.002 * rng.normal(size=shape)
    z[(u // 9 + v // 5) % 3 == 0] += 0.3
    drop = rng.random(shape) >= density
    if dtype == np.uint16:
        img = np.round(z * 1000.0).astype(np.uint16)
        img[drop] = 0
        return img
    img = z.astype(np.float32)
    img[drop] = BAD[rng.integers(0, len(BAD), size=int(drop.sum()))]
    return img


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


@pytest.mark.parametrize("radius", range(0, 9))
def test_vectorised_form_equals_the_pixel_loops_at_every_radius_and_min_support(radius):
    rng = np.random.default_rng(100 + radius)
    shape = (24, 40) if radius in (3, 8) else (11, 19)
    img = seeded(rng, shape)
    kw = dict(radius=radius, min_support=radius, range_abs=0.02)          # min_support 0..8 along with the radius
    got, want = F.filter_depth(img, **kw), F.filter_depth_loops(img, **kw)
    assert same(got, want), (radius, got[1], want[1])
    assert got[1]["n_kept"] == got[1]["n_unsupported"] + got[1]["n_written"] == int(N.keep_mask(img).sum())
    assert np.array_equal(got[0] != 0, F.supported_mask(img, N.keep_mask(img), 0.01, 0.0, radius))


def test_quad_terms_cuts_and_u16_equal_the_pixel_loops():
    rng = np.random.default_rng(120)
    img = seeded(rng, (13, 23))
    for kw in (dict(range_quad=0.01), dict(support_quad=0.02, support_abs=0.0), dict(range_quad=0.004, support_quad=0.004, radius=4),
               dict(z_min=1.0, z_max=1.3), dict(min_support=8, radius=2)):
        assert same(F.filter_depth(img, **kw), F.filter_depth_loops(img, **kw)), kw
    u16 = seeded(rng, (13, 23), dtype=np.uint16)
    for kw in (dict(depth_scale=0.001), dict(depth_scale=0.000125, range_quad=0.5, radius=2), dict(depth_scale=0.001, z_min=1.0, z_max=1.25)):
        got = F.filter_depth(u16, **kw)
        assert same(got, F.filter_depth_loops(u16, **kw)), kw
        assert 0 < got[1]["n_unsupported"] < got[1]["n_kept"]


def test_support_threshold_closure():
    """fabs(Zq - Zp) == S supports, one ulp further does not: zp 1.0, zq 1.0078125, support_abs 0.0078125 are exact in float32"""
    zq = np.float32(1.0078125)
    for q, supports in ((zq, True), (np.nextafter(zq, np.float32(2)), False)):
        img = np.full((3, 3), np.float32(1.0))
        img[0, 0] = q
        out, st = F.filter_depth(img, support_abs=0.0078125, min_support=8, radius=0)
        assert same((out, st), F.filter_depth_loops(img, support_abs=0.0078125, min_support=8, radius=0))
        assert (out[1, 1] == np.float32(1.0)) == supports and (out[1, 1] == 0) == (not supports)
        assert st["n_kept"] == 9


def test_range_threshold_closure():
    """|Zq - Zp| == R gives t = 1, k = 0: skipped, as is everything beyond; at half of R the weight is (3/4)^2 (3/4)^2"""
    far, half = np.float32(1.0078125), np.float32(1.00390625)
    for q in (far, np.nextafter(far, np.float32(2)), half):
        img = np.array([[1.0, q]], np.float32)
        out, st = F.filter_depth(img, range_abs=0.0078125, min_support=0, radius=1)
        assert same((out, st), F.filter_depth_loops(img, range_abs=0.0078125, min_support=0, radius=1))
        assert st == dict(n_kept=2, n_unsupported=0, n_written=2)
        if q != half:
            assert out.tobytes() == img.tobytes()
        else:
            w = 0.5625 * 0.5625
            assert out[0, 0] == np.float32((1.0 + w * float(half)) / (1.0 + w)) and out[0, 0] != np.float32(1.0)
            assert out[0, 1] == np.float32((w * 1.0 + float(half)) / (w + 1.0))


def test_constant_image_comes_back_at_min_support_8():
    """the border rule: a neighbour outside the image supports"""
    img = np.full((20, 30), np.float32(0.8125))
    for radius in (0, 3, 8):
        out, st = F.filter_depth(img, min_support=8, radius=radius)
        assert out.tobytes() == img.tobytes() and st == dict(n_kept=600, n_unsupported=0, n_written=600)


def step_image():
    img = np.full((12, 16), np.float32(1.0))
    img[:, 8:] = np.float32(1.05)
    return img


def lone_image():
    img = np.full((9, 9), np.float32(1.0))
    img[4, 4] = np.float32(1.03)
    return img


def test_step_comes_back_byte_identical():
    """a pixel on a straight step has 5 supporting neighbours: up to min_support 5 nothing is removed, and no smoothing crosses
    the step (0.05 > range_abs: those taps weigh exactly 0); at the default 6 the two edge columns go, the image's first and
    last row excepted (3 neighbours outside + 3 inside), and every pixel that stays keeps its bytes"""
    img = step_image()
    for kw in (dict(min_support=5), dict(min_support=5, radius=8), dict(min_support=0, radius=1), dict(min_support=3)):
        out, st = F.filter_depth(img, **kw)
        assert out.tobytes() == img.tobytes() and st["n_unsupported"] == 0, kw
    out, st = F.filter_depth(img)
    want = img.copy()
    want[1:-1, 7:9] = 0
    assert out.tobytes() == want.tobytes() and st == dict(n_kept=192, n_unsupported=20, n_written=172)


def test_lone_pixel_is_removed_and_its_neighbours_stay():
    out, st = F.filter_depth(lone_image())
    assert st == dict(n_kept=81, n_unsupported=1, n_written=80)
    want = np.full((9, 9), np.float32(1.0))
    want[4, 4] = 0
    assert out.tobytes() == want.tobytes()


def test_radius_0_returns_the_supported_pixels_bytes():
    rng = np.random.default_rng(121)
    for img, scale in ((seeded(rng, (24, 40)), 0.001), (seeded(rng, (24, 40), dtype=np.uint16), 0.000125)):
        z = N.metric_depth(img, scale)
        sup = F.supported_mask(z, N.keep_mask(z), 0.01, 0.0, 6)
        out, st = F.filter_depth(img, depth_scale=scale, radius=0)
        assert 0 < st["n_unsupported"] < st["n_kept"]
        assert out.tobytes() == np.where(sup, z, np.float32(0)).astype(np.float32).tobytes()


@pytest.fixture(scope="module")
def c1():
    _, depth, _, intr = D.c1_frame()
    return depth, intr


@pytest.fixture(scope="module")
def c1_filtered(c1):
    return F.filter_depth(c1[0])


def test_reference_frame_counts(c1, c1_filtered):
    depth, _ = c1
    assert c1_filtered[1] == dict(n_kept=166718, n_unsupported=6591, n_written=160127)
    for kw, want in ((dict(min_support=0), (166718, 0, 166718)), (dict(min_support=8), (166718, 11592, 155126)),
                     (dict(radius=4, range_quad=0.004, support_quad=0.004), (166718, 4762, 161956))):
        st = F.filter_depth(depth, **kw)[1]
        assert (st["n_kept"], st["n_unsupported"], st["n_written"]) == want, kw
    u16 = np.round(depth.astype(np.float64) * 1000.0).astype(np.uint16)
    assert F.filter_depth(u16)[1] == dict(n_kept=166718, n_unsupported=6583, n_written=160135)


def test_reference_frame_downstream_figures(c1, c1_filtered):
    """what the filter is for: the rows EdgeExtraction(0.03) keeps, and the rows without a normal, before and after"""
    depth, intr = c1
    out = c1_filtered[0]
    figures = []
    for img in (depth, out):
        rows, curv = N.depth_normals(img, intr, fp64=True)
        with np.errstate(invalid="ignore"):
            figures.append((rows.shape[0], int((curv > np.float32(0.03)).sum()), int(np.isnan(curv).sum()), float(np.nanmedian(curv))))
    assert [f[:3] for f in figures] == [(166718, 5000, 12), (160127, 1178, 4)]
    assert abs(figures[0][3] - 0.00515) < 5e-6 and abs(figures[1][3] - 0.00195) < 5e-6      # the medians DESIGN.md §23 records
    written = out > 0
    dz = np.abs(out[written].astype(np.float64) - depth[written].astype(np.float64))
    assert dz.max() < 0.01                                      # no tap beyond range_abs weighs: the mean cannot leave it
    assert abs(dz.max() - 0.0036) < 5e-5 and abs(dz.mean() - 0.00029) < 5e-6                 # as recorded in §23
