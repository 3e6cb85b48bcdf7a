"""The depth registration specification without a GPU: the host entries ppf_camera_project / _unproject / _map_boxes equal
tests/register_oracle.py byte for byte (every pixel of both fixture cameras, special values), and the oracle itself is held
to properties that do not depend on our restatement: a plane seen through both distorted lenses must come out at its
analytic depth along each colour pixel's own ray, without holes, and a box in front of it must stay separate and win."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import register_oracle as O
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.cloud_processor import camera, camera_points, map_boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DCAM, DROWS, DCOLS = O.DEPTH_CAM
CCAM, CROWS, CCOLS = O.COLOR_CAM
R, T = O.extrinsics()


def test_constants_agree_with_the_header():
    text = open(os.path.join(ROOT, "include", "ppf_hip.h")).read()
    assert int(re.search(r"#define PPF_CAMERA_NEWTON_ITERS (\d+)", text).group(1)) == O.NEWTON_ITERS == _capi.PPF_CAMERA_NEWTON_ITERS
    assert int(re.search(r"#define PPF_REGISTER_MAX_QUAD_PX (\d+)", text).group(1)) == O.MAX_QUAD_PX == _capi.PPF_REGISTER_MAX_QUAD_PX
    math = open(os.path.join(ROOT, "include", "ppf_camera_math.h")).read()
    assert float(re.search(r"#define PPF_CAMERA_MAX_RESIDUAL (\S+)", math).group(1)) == O.MAX_RESIDUAL


@pytest.mark.parametrize("which", ["depth", "colour"])
def test_camera_entries_equal_the_oracle_on_every_pixel(which):
    cam, rows, cols = O.DEPTH_CAM if which == "depth" else O.COLOR_CAM
    uu, vv = O.pixel_grid(rows, cols)
    uv = np.stack([uu, vv], axis=-1).reshape(-1, 2)
    xy, ok = camera_points(cam, uv, unproject=True)
    x, y, wok = O.unproject(cam, uu, vv)
    assert ok.all() and wok.all()                      # Newton converges from every pixel of the fixtures
    assert xy.tobytes() == np.stack([x, y], axis=-1).tobytes()
    back, ok2 = camera_points(cam, xy)
    u, v, wok2 = O.project(cam, xy[:, 0], xy[:, 1])
    assert ok2.all() and back.tobytes() == np.stack([u, v], axis=-1).tobytes()
    err = np.abs(back - uv).max()
    print(f"{which}: round trip {err:.3e} px")
    assert err < 1e-9


def test_camera_entries_equal_the_oracle_on_special_values():
    cam = DCAM.scaled(1.0, DCAM.cx, DCAM.cy)
    cam.max_r = 0.9
    zero_b = O.Cam(50.0, 50.0, 10.0, 10.0, (0.0, 0.0, 0.0, -4.0, 0.0, 0.0))   # b = 1 - 4 r2 == 0 at r2 = 0.25
    pts = np.array([[np.nan, 0.0], [0.0, np.nan], [np.inf, 0.0], [-np.inf, np.inf], [0.7, 0.7], [0.5, 0.0], [0.0, 0.5], [0.3, -0.4],
                    [1e200, 1e200], [0.0, 0.0], [-0.0, 0.1]])
    for c in (cam, zero_b, O.Cam(61.0, -60.5, 20.25, 15.5)):
        got, ok = camera_points(c, pts)
        u, v, wok = O.project(c, pts[:, 0], pts[:, 1])
        assert got.tobytes() == np.stack([u, v], axis=-1).tobytes() and (ok == wok).all()
        assert np.isnan(got[~ok]).all() and not ok[:4].any()
        px = np.concatenate([pts * 50.0, [[1e300, 0.0], [31.0, 27.0]]])
        got, ok = camera_points(c, px, unproject=True)
        x, y, wok = O.unproject(c, px[:, 0], px[:, 1])
        assert got.tobytes() == np.stack([x, y], axis=-1).tobytes() and (ok == wok).all()
        assert np.isnan(got[~ok]).all() and not ok[:4].any()
    ok = camera_points(cam, pts)[1]
    assert not ok[4] and ok[7]                         # (0.7, 0.7) is over max_r 0.9, (0.3, -0.4) is not
    ok = camera_points(zero_b, pts)[1]
    assert not ok[5] and not ok[6] and ok[9]           # b == 0 on the circle r2 = 0.25


def test_map_boxes_identity_clamp_and_invalid():
    pin = O.Cam(64.0, 64.0, 32.5, 24.25)               # dyadic values: the pinhole round trip is exact
    boxes = np.array([[3, 4, 10, 7], [0, 0, 64, 48], [20, 30, 1, 1], [-5, -6, 20, 20], [50, 40, 30, 30], [100, 100, 5, 5], [5, 5, 0, 3]], np.int32)
    got = map_boxes(pin, pin, 48, 64, boxes)
    assert got.tobytes() == O.map_boxes(pin, pin, 48, 64, boxes).tobytes()
    assert got[:3].tolist() == boxes[:3].tolist()      # interior boxes: the identity
    assert got[3].tolist() == [0, 0, 15, 14] and got[4].tolist() == [50, 40, 14, 8]   # across the edge: clamped
    assert got[5].tolist() == [0, 0, 0, 0] and got[6].tolist() == [0, 0, 0, 0]        # outside; empty
    # the distorted colour camera into a pinhole with its intrinsics: the oracle's boxes, and each contains the centre's image
    raw, to = CCAM, O.Cam(CCAM.fx, CCAM.fy, CCAM.cx, CCAM.cy)
    boxes = np.array([[10, 10, 30, 20], [60, 40, 50, 45], [0, 0, 120, 90], [100, 70, 40, 40]], np.int32)
    got = map_boxes(raw, to, CROWS, CCOLS, boxes)
    assert got.tobytes() == O.map_boxes(raw, to, CROWS, CCOLS, boxes).tobytes()
    for b, g in zip(boxes[:2], got[:2]):
        x, y, _ = O.unproject(raw, b[0] + b[2] / 2.0, b[1] + b[3] / 2.0)
        u, v, _ = O.project(to, x, y)
        assert g[0] <= u <= g[0] + g[2] and g[1] <= v <= g[1] + g[3]
    # every point invalid: a max_r below every point of the box
    tiny = CCAM.scaled(1.0, CCAM.cx, CCAM.cy)
    tiny.max_r = 0.05
    assert map_boxes(tiny, to, CROWS, CCOLS, [[0, 0, 20, 20]]).tolist() == [[0, 0, 0, 0]]
    assert map_boxes(raw, to, CROWS, CCOLS, np.zeros((0, 4), np.int32)).shape == (0, 4)


@pytest.fixture(scope="module")
def plane_run():
    z = O.plane_depth(DCAM, DROWS, DCOLS)
    return (z,) + O.register(z, DCAM, CCAM, CROWS, CCOLS, R, T)


def test_plane_comes_out_at_its_analytic_depth(plane_run):
    """Measured with this oracle on 90 x 120: largest difference 3.66e-5 m, mean 4.28e-6 m, 52.5 % of the image filled, no
    holes, largest triangle box 4 px.  The bound is twice the largest difference: float rounding of zc and the chord error of
    a 2-pixel triangle on a plane seen through a distorted lens, both properties of the specification."""
    z, img, cnt, info = plane_run
    want = O.plane_analytic(CCAM, CROWS, CCOLS, R, T)
    f = img > 0
    err = np.abs(img[f].astype(np.float64) - want[f])
    print(f"plane: max {err.max():.3e} m, mean {err.mean():.3e} m, filled {f.mean():.4f}, max box {info['max_box']}, counters {cnt}")
    assert err.max() <= 2 * 3.67e-5
    assert 0.45 < f.mean() < 0.60                      # the depth camera's field ends inside the colour image
    assert cnt["n_filled"] == int(f.sum()) and cnt["n_vertices"] == DROWS * DCOLS and cnt["n_quads"] == (DROWS - 1) * (DCOLS - 1)
    assert cnt["n_quads_cut"] == 0 and cnt["n_quads_oversize"] == 0 and info["max_box"] <= 4
    e = ~f
    holes = e[1:-1, 1:-1] & f[:-2, 1:-1] & f[2:, 1:-1] & f[1:-1, :-2] & f[1:-1, 2:]
    assert not holes.any()                             # no empty pixel with four filled 4-neighbours


def test_box_in_front_of_the_plane_is_cut_and_wins(plane_run):
    zb = O.plane_with_box(DCAM, DROWS, DCOLS)
    r0, r1, c0, c1 = O.BOX_RECT
    img, cnt, _ = O.register(zb, DCAM, CCAM, CROWS, CCOLS, R, T)
    only_box = np.zeros_like(zb)
    only_box[r0:r1, c0:c1] = zb[r0:r1, c0:c1]
    rest = zb.copy()
    rest[r0:r1, c0:c1] = 0
    img_box = O.register(only_box, DCAM, CCAM, CROWS, CCOLS, R, T)[0]
    img_rest = O.register(rest, DCAM, CCAM, CROWS, CCOLS, R, T)[0]
    fb, fr = img_box > 0, img_rest > 0
    box_hi, rest_lo = float(img_box[fb].max()), float(img_rest[fr].min())
    assert box_hi + 0.3 < rest_lo                      # the two depth ranges are disjoint in the colour frame
    assert cnt["n_quads_cut"] > 0
    f = img > 0
    assert not ((img[f] > box_hi) & (img[f] < rest_lo)).any()      # nothing interpolated across the discontinuity
    both = fb & fr
    assert both.sum() > 20                             # parallax: the box covers plane the depth camera still sees
    assert img[fb].tobytes() == img_box[fb].tobytes()  # where both project, the nearer wins
    assert img[fr & ~fb].tobytes() == img_rest[fr & ~fb].tobytes() and (f == (fb | fr)).all()


def test_camera_record_from_every_form():
    c = camera(DCAM)
    assert [getattr(c, f) for f in O.Cam.FIELDS] == DCAM.values() and list(c.reserved) == [0.0, 0.0, 0.0]
    d = camera(dict(fx=1.0, fy=2.0, cx=3.0, cy=4.0, k3=0.5))
    assert (d.fx, d.fy, d.cx, d.cy, d.k3, d.k1) == (1.0, 2.0, 3.0, 4.0, 0.5, 0.0)
    e = camera(np.array([[5.0, 0, 7.0], [0, 6.0, 8.0], [0, 0, 1]]))
    assert (e.fx, e.fy, e.cx, e.cy) == (5.0, 6.0, 7.0, 8.0)
    assert camera(c) is c
    assert C.sizeof(c) == 16 * 8
