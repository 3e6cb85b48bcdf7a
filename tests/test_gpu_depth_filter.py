"""ppf_depth_filter on the device against the numpy oracle (tests/depth_filter_oracle.py), the image byte for byte and the
three counts: shapes across the kernel's tile edges in both directions, seeded content with holes and non-finite values, both
formats, a pitched input, every radius and min_support, the quad terms, the two threshold closures, images with a known
answer, unsupported pixels on the tile edges and in the halo, the host and the device entry, ``out=``, repeated and concurrent
calls, a window of the C1 frame through the filter into the normals, ``from_depth(filter=...)`` and the C++ demo."""
import os
import subprocess
import threading

import numpy as np
import pytest

import depth_filter_oracle as F
import depth_normals_oracle as N
import prep_data as D
from test_depth_filter_oracle import lone_image, seeded, step_image
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, filter_depth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
TILE_W, TILE_H = 64, 4     # k_depth_filter's tile (ppf_filter_kernels.h)
DEPTH_KEYS = ("depth_scale", "z_min", "z_max")
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 3), (4, 64), (5, 65), (9, 129), (37, 200)]


def split(kw):
    return {k: v for k, v in kw.items() if k in DEPTH_KEYS}, {k: v for k, v in kw.items() if k not in DEPTH_KEYS}


def check_equal(img, **kw):
    """the device's image and counts are the oracle's; returns the oracle's (image, counts)"""
    dk, fk = split(kw)
    want, counts = F.filter_depth(img, **kw)
    got, st = filter_depth(img, params=fk, return_stats=True, **dk)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert {k: st[k] for k in counts} == counts, (img.shape, kw, st, counts)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        v, u = bad[0]
        raise AssertionError(f"{img.shape} {kw}: {len(bad)} pixels differ, first ({v}, {u}): {got[v, u]!r} against {want[v, u]!r}")
    return want, counts


def test_shapes_across_the_tile_edges_both_formats():
    rng = np.random.default_rng(31)
    for shape in SHAPES:
        check_equal(seeded(rng, shape), range_abs=0.02)
        check_equal(seeded(rng, shape, dtype=np.uint16), radius=2)
    _, counts = check_equal(seeded(rng, (37, 200)))
    assert counts["n_unsupported"] > 0 and counts["n_written"] > 0
    check_equal(seeded(rng, (9, 129), density=0.0))              # nothing kept: all zeros
    check_equal(seeded(rng, (9, 129), density=1.0), z_min=1.0, z_max=1.25)


def test_every_radius_and_every_min_support():
    rng = np.random.default_rng(32)
    img = seeded(rng, (21, 131))
    for radius in range(0, 9):
        check_equal(img, radius=radius, min_support=radius, range_abs=0.02)
    u16 = seeded(rng, (9, 70), dtype=np.uint16)
    for min_support in range(0, 9):
        check_equal(u16, radius=8 - min_support, min_support=min_support, depth_scale=0.000125, range_abs=0.004, support_abs=0.002)


def test_quad_terms_and_pitched_inputs():
    rng = np.random.default_rng(33)
    shape = (13, 141)
    img = seeded(rng, shape)
    for kw in (dict(range_quad=0.01), dict(support_quad=0.02, support_abs=0.0), dict(radius=4, range_quad=0.004, support_quad=0.004)):
        check_equal(img, **kw)
    wide = seeded(rng, (shape[0], shape[1] + 37))
    view = wide[:, 5:5 + shape[1]]
    assert view.strides[0] > shape[1] * 4
    check_equal(view)
    wide16 = seeded(rng, (shape[0], shape[1] + 3), dtype=np.uint16)
    check_equal(wide16[:, 2:2 + shape[1]], support_quad=0.01)


def test_threshold_closures():
    zq = np.float32(1.0078125)
    for q, supports in ((zq, True), (np.nextafter(zq, np.float32(2)), False)):
        img = np.full((3, 3), np.float32(1.0))
        img[0, 0] = q
        out, _ = check_equal(img, support_abs=0.0078125, min_support=8, radius=0)
        assert (out[1, 1] == np.float32(1.0)) == supports
    for q in (zq, np.nextafter(zq, np.float32(2)), np.float32(1.00390625)):
        img = np.array([[1.0, q]], np.float32)
        out, _ = check_equal(img, range_abs=0.0078125, min_support=0, radius=1)
        assert (out.tobytes() == img.tobytes()) == (q >= zq)


def test_images_with_a_known_answer():
    const = np.full((20, 30), np.float32(0.8125))
    out, counts = check_equal(const, min_support=8)
    assert out.tobytes() == const.tobytes() and counts["n_unsupported"] == 0        # the border rule
    out, _ = check_equal(step_image(), min_support=5, radius=8)
    assert out.tobytes() == step_image().tobytes()
    check_equal(step_image())
    out, counts = check_equal(lone_image())
    assert counts == dict(n_kept=81, n_unsupported=1, n_written=80) and out[4, 4] == 0 and (out[3:6, 3:6].sum() == 8.0)


def spiked(shape, spikes):
    """a gentle ramp (every tap inside the default range, so a missing tap changes the mean) with isolated pixels 5 cm in
    front of it: each is unsupported and costs its eight neighbours one supporter"""
    v, u = np.mgrid[0:shape[0], 0:shape[1]]
    img = (1.0 + 0.0004 * u + 0.0007 * v).astype(np.float32)
    for sv, su in spikes:
        img[sv, su] -= np.float32(0.05)
    return img


def test_unsupported_pixels_on_the_tile_edges_and_in_the_halo():
    """the halo must know the support of its pixels: spikes on both sides of a tile edge in u (63 | 64) and v (3 | 4), and
    exactly radius and radius + 1 pixels outside a tile in all four directions; at min_support 8 a spike in the extra ring
    makes the outermost halo pixel unsupported"""
    shape = (30, 150)
    assert shape[1] > 2 * TILE_W and shape[0] > 4 * TILE_H
    edges = [(1, 63), (9, 64), (3, 20), (4, 30), (21, 63), (28, 64)]
    for radius in (1, 3, 8):
        halo = [(5, 63 + radius), (13, 63 + radius + 1), (17, 64 - radius), (25, 64 - radius - 1),       # right of tile 0, left of tile 1
                (15 + radius, 10), (15 + radius + 1, 40), (12 - radius, 100), (12 - radius - 1, 120)]   # below and above tile row 3
        img = spiked(shape, edges + halo)
        for min_support in (6, 8):
            _, counts = check_equal(img, radius=radius, min_support=min_support)
            assert counts["n_unsupported"] == len(edges + halo) * (9 if min_support == 8 else 1)


def test_host_and_device_entries_give_the_same_bytes_and_out_is_reused():
    import torch
    rng = np.random.default_rng(34)
    shape = (37, 200)
    img = seeded(rng, shape)
    want, counts = check_equal(img)
    t = torch.from_numpy(img).cuda()
    got, st = filter_depth(t, return_stats=True)
    assert got.is_cuda and got.dtype == torch.float32 and got.cpu().numpy().tobytes() == want.tobytes()
    assert {k: st[k] for k in counts} == counts
    out = torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert filter_depth(t, out=out) is out
    assert out.cpu().numpy().tobytes() == want.tobytes()
    wide = torch.from_numpy(np.ascontiguousarray(np.pad(img, ((0, 0), (8, 16)), constant_values=1.0))).cuda()      # a strided tensor
    view = wide[:, 8:8 + shape[1]]
    assert not view.is_contiguous() and filter_depth(view, out=out) is out and out.cpu().numpy().tobytes() == want.tobytes()
    u16 = seeded(rng, shape, dtype=np.uint16)
    want16, _ = check_equal(u16, depth_scale=0.000125, radius=5)
    assert filter_depth(torch.from_numpy(u16).cuda(), depth_scale=0.000125, params=dict(radius=5)).cpu().numpy().tobytes() == want16.tobytes()
    host_out = np.full(shape, np.float32(7.0))
    assert filter_depth(img, out=host_out) is host_out and host_out.tobytes() == want.tobytes()
    # the output must not overlap the image, and must be what it says
    n = shape[0] * shape[1]
    buf = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    for call in (lambda: filter_depth(buf[:n].view(shape), out=buf[n // 2:n // 2 + n].view(shape)),
                 lambda: filter_depth(buf[:n].view(shape), out=buf[:n].view(shape)),
                 lambda: filter_depth(t, out=torch.zeros((shape[0], shape[1] + 1), dtype=torch.float32, device="cuda")),
                 lambda: filter_depth(t, out=torch.zeros(shape, dtype=torch.float32))):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID
    assert filter_depth(buf[:n].view(shape), out=buf[n:].view(shape)) is not None          # side by side is fine
    torch.cuda.synchronize()


def test_launches_and_waits_do_not_depend_on_the_content():
    rng = np.random.default_rng(35)
    shape = (37, 200)
    stats = [filter_depth(img, return_stats=True)[1] for img in (seeded(rng, shape, 0.3), np.full(shape, np.float32(1.0)), np.zeros(shape, np.float32))]
    assert len({st["n_written"] for st in stats}) == 3
    assert [(st["n_launches"], st["n_host_syncs"]) for st in stats] == [(1, 1)] * 3


def test_two_concurrent_callers():
    rng = np.random.default_rng(36)
    imgs = [seeded(rng, (60, 300)), seeded(rng, (60, 300), 0.6)]
    want = [check_equal(img, radius=4)[0].tobytes() for img in imgs]
    got = [None, None]

    def work(j):
        got[j] = [filter_depth(imgs[j], params=dict(radius=4)).tobytes() for _ in range(3)]
    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(g == want[j] for j in range(2) for g in got[j])


def test_c1_window_through_the_filter_into_the_normals():
    import torch
    _, depth, box, intr = D.c1_frame()
    x, y, w, h = box
    r0 = int(np.clip(y + h // 2 - 80, 0, depth.shape[0] - 160))
    c0 = int(np.clip(x + w // 2 - 112, 0, depth.shape[1] - 224))
    win = np.ascontiguousarray(depth[r0:r0 + 160, c0:c0 + 224])
    shifted = (intr[0], intr[1], intr[2] - c0, intr[3] - r0)
    want_img, counts = check_equal(win)
    assert counts["n_kept"] > 10000 and counts["n_unsupported"] > 100
    want_rows, want_curv = N.depth_normals(want_img, shifted, fp64=True)
    t = torch.from_numpy(win).cuda()
    filtered = filter_depth(t)
    assert filtered.is_cuda
    rows, curv = DeviceCloud.from_depth(filtered, shifted, fp64=True, normals={}).download()
    assert rows.tobytes() == want_rows.tobytes() and curv.tobytes() == want_curv.tobytes()
    # from_depth(filter=...) is the two calls, on a tensor and on an array, with and without parameters
    for src in (t, win):
        rows, curv = DeviceCloud.from_depth(src, shifted, fp64=True, normals={}, filter={}).download()
        assert rows.tobytes() == want_rows.tobytes() and curv.tobytes() == want_curv.tobytes()
    prm = dict(radius=2, min_support=7)
    two = DeviceCloud.from_depth(filter_depth(t, params=prm, z_min=0.5), shifted, z_min=0.5).download()
    one = DeviceCloud.from_depth(t, shifted, z_min=0.5, filter=prm).download()
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
    assert one[0].shape[0] == int(N.keep_mask(F.filter_depth(win, z_min=0.5, **prm)[0], 0.5).sum()) > 10000
    plain = DeviceCloud.from_depth(t, shifted).download()
    assert plain[0].shape[0] == counts["n_kept"]                      # filter=None changes nothing
    cp = CloudProcessor(None, win, [], [], [], 0.05, 0.05)
    assert cp.FilterDepth().tobytes() == want_img.tobytes() and cp.depth_filter_stats["n_unsupported"] == counts["n_unsupported"]


def words(a):
    return int(np.ascontiguousarray(a).view(np.uint32).astype(np.uint64).sum())


def test_cpp_demo_matches_the_python_route(tmp_path, bottle):
    from test_gpu_frame import _render_frame
    _, depth, _, K, _, _ = _render_frame(bottle)
    depth = np.ascontiguousarray(depth, np.float32)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    exe = str(tmp_path / "depth_filter_demo")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "depth_filter_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    (tmp_path / "depth.f32").write_bytes(depth.tobytes())
    for prm in (dict(), dict(radius=5, range_abs=0.02, range_quad=0.01, support_abs=0.005, support_quad=0.002, min_support=7)):
        full = dict(F.DEFAULTS, **prm)
        args = [repr(float(full[k])) if "_" in k and k != "min_support" else str(full[k])
                for k in ("radius", "range_abs", "range_quad", "support_abs", "support_quad", "min_support")]
        r = subprocess.run([exe, str(tmp_path / "depth.f32"), str(depth.shape[0]), str(depth.shape[1])] + [repr(float(v)) for v in intr] + args + ["0.03"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        filtered, st = filter_depth(depth, params=prm, return_stats=True)
        want = [f"kept {st['n_kept']} unsupported {st['n_unsupported']} written {st['n_written']}"]
        for name, img in (("raw", depth), ("filtered", filtered)):
            rows, curv = DeviceCloud.from_depth(img, intr, fp64=True, normals={}).download()
            with np.errstate(invalid="ignore"):
                over = int((curv > np.float32(0.03)).sum())
            want.append(f"{name} image checksum {words(img)} cloud rows {rows.shape[0]} over {over} checksum {words(rows) + words(curv)}")
        assert r.stdout.strip().splitlines() == want
        assert st["n_written"] > 0
