"""ppf_cloud_from_depth_normals on the device against the numpy oracle (tests/depth_normals_oracle.py), rows and curvature
byte for byte, NaNs as bytes: small shapes, every width and height across the kernel's tile and halo boundaries, radii,
densities with invalid values, cuts, formats, pitches, both back-projection modes, the min_neighbours and depth-change
thresholds, degenerate neighbourhoods, the drop flag, the device entry on a strided tensor and a side stream, repeated and
concurrent calls, a window of the C1 frame, the later stages carrying the normals, and the C++ demo."""
import os
import subprocess
import threading

import numpy as np
import pytest

import depth_normals_oracle as O
import prep_data as D
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
NORMAL_KEYS = ("radius", "max_depth_change", "min_neighbours", "drop")
TILE_W, TILE_H = 64, 4     # k_depth_normals' tile (ppf_depth_normals_kernels.h): the sweeps below cover twice that and more


def split(kw):
    nk = {k: kw[k] for k in NORMAL_KEYS if k in kw}
    return {k: v for k, v in kw.items() if k not in NORMAL_KEYS}, nk


def device(img, intr, **kw):
    dk, nk = split(kw)
    return DeviceCloud.from_depth(img, intr, normals=nk, **dk).download()


def check_equal(img, intr, **kw):
    """the device's rows and curvature are the oracle's bytes; returns the oracle's (rows, curvature)"""
    dk, nk = split(kw)
    want_rows, want_curv = O.depth_normals(img, intr, **dk, **nk)
    rows, curv = device(img, intr, **kw)
    assert rows.shape == want_rows.shape, (img.shape, kw, rows.shape, want_rows.shape)
    if rows.tobytes() != want_rows.tobytes() or curv.tobytes() != want_curv.tobytes():
        bad = np.flatnonzero((rows.view(np.uint32) != want_rows.view(np.uint32)).any(axis=1) | (curv.view(np.uint32) != want_curv.view(np.uint32)))
        raise AssertionError(f"{img.shape} {kw}: {bad.size} of {rows.shape[0]} rows differ, first {bad[0]}: {rows[bad[0]]} {curv[bad[0]]} "
                             f"against {want_rows[bad[0]]} {want_curv[bad[0]]}")
    return want_rows, want_curv


def surface(rng, shape, density=1.0, dtype=np.float32, specials=True):
    """a smooth surface with a little noise and a depth step, so that windows hold between 1 and all of their pixels; the
    dropped pixels are the invalid values of test_gpu_depth.py"""
    rows, cols = shape
    v, u = np.mgrid[0:rows, 0:cols]
    z = 1.0 + 0.3 * np.sin(u / 7.0) + 0.2 * np.cos(v / 5.0) + 0.002 * rng.normal(size=shape)
    z[(u // 11 + v // 6) % 3 == 0] += 0.4                      # steps far above any max_depth_change used here
    drop = rng.random(shape) >= density
    if dtype == np.uint16:
        img = np.round(z * 1000.0).astype(np.uint16)
        img[drop] = 0
        return img
    img = z.astype(np.float32)
    if specials:
        bad = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -0.5, -1e-30], np.float32)
        img[drop] = bad[rng.integers(0, len(bad), size=int(drop.sum()))]
    else:
        img[drop] = 0
    return img


def intr_for(rng, shape):
    return (rng.uniform(300, 1200), rng.uniform(300, 1200), rng.uniform(0, shape[1]), rng.uniform(0, shape[0]))


def test_small_shapes():
    rng = np.random.default_rng(21)
    for shape in [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3)]:
        for fp64 in (False, True):
            check_equal(surface(rng, shape), intr_for(rng, shape), radius=1, fp64=fp64, max_depth_change=0.05)
    for shape in [(17, 121), (33, 31), (64, 257)]:
        img = surface(rng, shape, 0.9)
        rows, curv = check_equal(img, intr_for(rng, shape), fp64=True)
        assert 0 < int(np.isnan(curv).sum()) < rows.shape[0] // 2      # both kinds of row are present


def test_every_width_and_height_across_the_tile_and_halo_boundaries():
    rng = np.random.default_rng(22)
    assert 130 >= 2 * TILE_W and 40 >= 2 * TILE_H
    for width in range(1, 131):
        shape = (9, width)
        check_equal(surface(rng, shape, 0.95), intr_for(rng, shape), radius=3, fp64=bool(width & 1))
    for height in range(1, 41):
        shape = (height, 9)
        check_equal(surface(rng, shape, 0.95), intr_for(rng, shape), radius=3, fp64=bool(height & 1))


def test_radii_densities_and_invalid_values():
    rng = np.random.default_rng(23)
    for shape in [(41, 150), (13, 70)]:
        intr = intr_for(rng, shape)
        for density in (0.0, 0.001, 0.5, 1.0):
            img = surface(rng, shape, density)
            for radius in (1, 8):
                rows, _ = check_equal(img, intr, radius=radius, fp64=bool(radius & 1), max_depth_change=0.03)
                assert density > 0 or rows.shape[0] == 0


def test_cuts_formats_pitches_and_modes():
    rng = np.random.default_rng(24)
    shape = (37, 141)
    intr = intr_for(rng, shape)
    img = surface(rng, shape, 0.8)
    for z_min, z_max in ((0.9, 0.0), (0.0, 1.2), (0.95, 1.3), (2.0, 1.0), (1.0, 1.0)):   # a cut pixel is no neighbour
        check_equal(img, intr, z_min=z_min, z_max=z_max, fp64=bool(rng.integers(0, 2)))
    for scale in (0.001, 0.000125):
        u16 = surface(rng, shape, 0.8, np.uint16)
        for fp64 in (False, True):
            check_equal(u16, intr, depth_scale=scale, fp64=fp64)
        check_equal(u16, intr, depth_scale=scale, z_min=900 * scale, z_max=1300 * scale, radius=2)
        wide = surface(rng, (shape[0], shape[1] + 37), 0.8, np.uint16)       # a pitch wider than the row
        view = wide[:, 5:5 + shape[1]]
        assert view.strides[0] > shape[1] * 2
        check_equal(view, intr, depth_scale=scale)
    wide = surface(rng, (shape[0], shape[1] + 3), 0.8)
    for fp64 in (False, True):
        check_equal(wide[:, 2:2 + shape[1]], intr, fp64=fp64)
    check_equal(wide[:, 1:], intr)


def test_min_neighbours_at_k_and_one_above():
    rng = np.random.default_rng(25)
    shape = (12, 70)
    img, intr = surface(rng, shape, 1.0), intr_for(rng, shape)
    _, _, k = O.depth_normals(img, intr, radius=2, max_depth_change=0.02, return_k=True)
    row = int(np.flatnonzero((k >= 4) & (k < 25))[0])          # a pixel whose window is cut by a step or the border
    for mn, has_normal in ((int(k[row]), True), (int(k[row]) + 1, False)):
        rows, curv = check_equal(img, intr, radius=2, max_depth_change=0.02, min_neighbours=mn)
        assert bool(np.isfinite(rows[row, 3:]).all() and np.isfinite(curv[row])) == has_normal
        assert has_normal or (np.isnan(rows[row, 3:]).all() and np.isnan(curv[row]))
    check_equal(img, intr, radius=2, min_neighbours=25)        # only full windows
    check_equal(img, intr, radius=8, min_neighbours=289)


def test_depth_change_threshold_equality_is_a_neighbour():
    img = np.array([[1.0, 1.0, 1.0, 1.25, np.nextafter(np.float32(1.25), np.float32(2))]], np.float32)
    intr = (500.0, 500.0, 2.0, 0.0)
    for mn, none in ((3, [False] * 5), (4, [False] * 5), (5, [True, True, True, False, False])):
        rows, curv = check_equal(img, intr, radius=8, max_depth_change=0.25, min_neighbours=mn)
        assert np.isnan(curv).tolist() == none


def test_degenerate_neighbourhoods():
    intr = (600.0, 610.0, 31.5, 23.25)
    rows, curv = check_equal(np.full((20, 70), np.float32(0.75)), intr, radius=3, fp64=True)      # an exact plane z = const
    assert np.array_equal(rows[:, 3:], np.tile(np.float32([0, 0, -1]), (rows.shape[0], 1))) and not curv.any()
    rng = np.random.default_rng(26)
    line = (1.0 + 0.05 * np.sin(np.arange(200) / 9.0) + 0.001 * rng.normal(size=200)).astype(np.float32)[None, :]
    for fp64 in (False, True):                                 # collinear neighbours: whatever the Jacobi rule gives
        check_equal(line, (600.0, 610.0, 99.5, 0.0), radius=3, fp64=fp64, max_depth_change=0.05)
        check_equal(line, (600.0, 610.0, 99.5, 7.25), radius=8, fp64=fp64, max_depth_change=0.05)


def test_without_drop_the_rows_are_from_depths_and_with_drop_the_nan_rows_leave():
    rng = np.random.default_rng(27)
    shape = (45, 133)
    intr = intr_for(rng, shape)
    for img, dk in ((surface(rng, shape, 0.7), dict(fp64=True, z_min=0.9)), (surface(rng, shape, 0.7, np.uint16), dict(depth_scale=0.001))):
        plain = DeviceCloud.from_depth(img, intr, **dk).download()[0]
        rows, curv = check_equal(img, intr, **dk)
        assert rows.shape == plain.shape and rows[:, :3].tobytes() == plain[:, :3].tobytes()
        none = np.isnan(curv)
        assert 0 < int(none.sum()) < none.size
        got, gcurv = device(img, intr, drop=True, **dk)
        assert got.tobytes() == rows[~none].tobytes() and gcurv.tobytes() == curv[~none].tobytes()
        check_equal(img, intr, drop=True, min_neighbours=20, **dk)    # dropping never changes who is a neighbour
    empty = DeviceCloud.from_depth(np.zeros(shape, np.float32), intr, normals={})
    assert len(empty) == 0 and empty.download()[0].shape == (0, 6)
    lonely = np.zeros(shape, np.float32)
    lonely[7, 9] = 1.0
    assert len(DeviceCloud.from_depth(lonely, intr, normals=dict(drop=True))) == 0
    assert len(DeviceCloud.from_depth(lonely, intr, normals={})) == 1


def test_device_entry_strided_tensor_on_a_side_stream():
    import torch
    rng = np.random.default_rng(28)
    shape = (75, 210)
    intr = intr_for(rng, shape)
    wide = np.ones((shape[0], shape[1] + 24), np.float32)      # outside the window: must not be read into a neighbourhood
    wide[:, 8:8 + shape[1]] = surface(rng, shape, 0.8)
    t = torch.from_numpy(wide).cuda()[:, 8:8 + shape[1]]
    assert t.stride(0) == wide.shape[1] and not t.is_contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for kw in (dict(fp64=True), dict(radius=8, drop=True, min_neighbours=30)):
        want = check_equal(wide[:, 8:8 + shape[1]], intr, **kw)
        dk, nk = split(kw)
        with torch.cuda.stream(side):
            got = DeviceCloud.from_depth(t, intr, normals=nk, **dk).download()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    u16 = surface(rng, shape, 0.8, np.uint16)
    tu = torch.from_numpy(u16).cuda()
    want = check_equal(u16[:, 3:], intr, depth_scale=0.000125)
    got = DeviceCloud.from_depth(tu[:, 3:], intr, depth_scale=0.000125, normals={}).download()
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    torch.cuda.synchronize()


def test_repeated_and_concurrent_calls_give_the_same_bytes():
    rng = np.random.default_rng(29)
    shape = (120, 300)
    img, intr = surface(rng, shape, 0.85), intr_for(rng, shape)

    def run():
        rows, curv = device(img, intr, fp64=True, radius=4)
        return rows.tobytes(), curv.tobytes()
    want = check_equal(img, intr, fp64=True, radius=4)
    first = run()
    assert first == (want[0].tobytes(), want[1].tobytes()) and run() == first
    got = [None, None]

    def work(j):
        got[j] = [run() for _ in range(3)]
    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(r == first for g in got for r in g)


def test_c1_window_around_the_box():
    _, depth, box, intr = D.c1_frame()
    x, y, w, h = box
    r0 = int(np.clip(y + h // 2 - 80, 0, depth.shape[0] - 160))
    c0 = int(np.clip(x + w // 2 - 112, 0, depth.shape[1] - 224))
    win = depth[r0:r0 + 160, c0:c0 + 224]
    assert int((win > 0).sum()) > 10000
    shifted = (intr[0], intr[1], intr[2] - c0, intr[3] - r0)
    for fp64 in (True, False):
        rows, curv = check_equal(win, shifted, fp64=fp64)
        assert int((curv > 0.03).sum()) > 100


def checksum(rows, curv):
    return int(rows.view(np.uint32).astype(np.uint64).sum() + curv.view(np.uint32).astype(np.uint64).sum())


@pytest.fixture(scope="module")
def rendered(bottle):
    from test_gpu_frame import _render_frame
    scene, depth, boxes, K, objs, solid = _render_frame(bottle)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    rows, curv = O.depth_normals(depth, intr, fp64=True)
    assert rows[:, :3].tobytes() == scene.tobytes()
    return depth, K, intr, rows, curv


def test_later_stages_carry_the_depth_normals(rendered):
    depth, K, intr, want_rows, want_curv = rendered
    cp = CloudProcessor(None, depth, [], [], [], 0.05, 0.05)
    scene = cp.Deprojection(K, fp64=True, normals=dict(radius=3))
    rows, curv = scene.download()
    assert rows.tobytes() == want_rows.tobytes() and curv.tobytes() == want_curv.tobytes()
    kept, plane_labels = scene.remove_planes(return_labels=True)
    kept_idx = np.flatnonzero(plane_labels == 0)
    assert len(kept) == kept_idx.size
    found, labels = kept.clusters(return_labels=True)
    assert len(found) == 3
    for k, cluster in enumerate(found):
        idx = kept_idx[np.flatnonzero(labels == k)]
        crows, ccurv = cluster.download()
        assert crows.tobytes() == want_rows[idx].tobytes() and ccurv.tobytes() == want_curv[idx].tobytes()
        with np.errstate(invalid="ignore"):
            edge = idx[want_curv[idx] > np.float32(0.03)]
        erows, ecurv = cluster.edges(0.03).download()
        assert 0 < edge.size < idx.size
        assert erows.tobytes() == want_rows[edge].tobytes() and ecurv.tobytes() == want_curv[edge].tobytes()


def test_cpp_demo_matches_the_python_route(tmp_path, rendered):
    depth, K, intr, _, _ = rendered
    exe = str(tmp_path / "depth_normals_demo")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "depth_normals_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    (tmp_path / "depth.f32").write_bytes(np.ascontiguousarray(depth, np.float32).tobytes())
    for radius, drop, fp64 in ((3, 0, 1), (2, 1, 0)):
        r = subprocess.run([exe, str(tmp_path / "depth.f32"), str(depth.shape[0]), str(depth.shape[1])] + [repr(float(v)) for v in intr] +
                           [str(radius), "0.02", "3", str(drop), str(fp64), "0.03"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        scene = DeviceCloud.from_depth(depth, intr, fp64=bool(fp64), normals=dict(radius=radius, drop=bool(drop)))
        kept = scene.remove_planes()
        found = kept.clusters(intr=intr, image_size=depth.shape)
        want = [f"scene rows {len(scene)} checksum {checksum(*scene.download())}",
                f"plane-free rows {len(kept)} checksum {checksum(*kept.download())}", f"clusters {len(found)}"]
        for k, c in enumerate(found):
            e = c.edges(0.03)
            want.append(f"cluster {k}: rows {len(c)} checksum {checksum(*c.download())} edge rows {len(e)} checksum {checksum(*e.download())}")
        assert r.stdout.strip().splitlines() == want
        assert len(found) == 3
