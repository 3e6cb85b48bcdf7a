"""ppf_depth_segments on the device against the numpy oracle (tests/depth_segments_oracle.py): the label image byte for byte,
the info rows, the counts and the four pixel counts of the stats.  Shapes across the kernels' tile edges in both directions,
seeded content with holes and non-finite values, both formats, a pitched input, chains that cross every tile edge many times
(a serpentine, a comb, a spiral, each also cut in the middle), a component that reaches a tile through two neighbour tiles,
the chessboard, the threshold closures, normals with NaNs and border pixels at the tile edges, the ranking at its capacity, the
host and the device entry, ``out=``, a side stream, launches that do not depend on the content, repeated and concurrent calls,
and the reference window through filter -> normals -> segments -> ProposeSegments and the C++ demo."""
import os
import subprocess
import threading

import numpy as np
import pytest

import depth_normals_oracle as N
import depth_segments_oracle as S
from test_depth_filter_oracle import seeded
from test_depth_segments_oracle import chessboard, plateaus, reference_window, seeded_normals, with_normals
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, filter_depth, segment_depth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
TW, TH = 64, 16            # the tile of k_seg_tile / k_seg_flatten (ppf_segment_kernels.h)
DEPTH_KEYS = ("depth_scale", "z_min", "z_max")
SHAPES = [(1, 1), (1, 7), (7, 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1), (37, 200)]
ONE = np.float32(1.0)


def cloud_of(normals):
    rows, curv = normals
    return DeviceCloud.upload(rows, curvature=curv) if len(rows) else DeviceCloud.upload(np.zeros((0, 6), np.float32))


def info_rows(info):
    return [dict(n_pixels=int(r["n_pixels"]), n_border=int(r["n_border"]), first_pixel=int(r["first_pixel"]),
                 box_xywh=tuple(int(v) for v in r["box_xywh"]), z_lo=np.float32(r["z_lo"]), z_hi=np.float32(r["z_hi"])) for r in info]


def check_equal(img, normals=None, **kw):
    """the device's labels, info, counts and pixel counts are the oracle's; returns the oracle's result and the device's stats"""
    dk = {k: v for k, v in kw.items() if k in DEPTH_KEYS}
    sk = {k: v for k, v in kw.items() if k not in DEPTH_KEYS}
    want = S.segments(img, normals=normals, **kw)
    cloud = cloud_of(normals) if normals is not None else None
    labels, info, counts, st = segment_depth(img, normals=cloud, params=sk, return_info=True, return_stats=True, **dk)
    assert labels.dtype == np.int32 and labels.shape == want[0].shape
    assert tuple(int(c) for c in counts) == want[2], (img.shape, kw, counts, want[2])
    assert {k: st[k] for k in want[3]} == want[3], (img.shape, kw, st, want[3])
    if labels.tobytes() != want[0].tobytes():
        bad = np.argwhere(labels != want[0])
        v, u = bad[0]
        raise AssertionError(f"{img.shape} {kw}: {len(bad)} labels differ, first ({v}, {u}): {labels[v, u]} against {want[0][v, u]}")
    assert info_rows(info) == want[1], (img.shape, kw)
    assert st["n_host_syncs"] == 1
    return want, st


def test_shapes_across_the_tile_edges_both_formats():
    rng = np.random.default_rng(241)
    for shape in SHAPES:
        for flags in (0, S.EIGHT):
            check_equal(seeded(rng, shape), min_size=1, flags=flags)
        check_equal(seeded(rng, shape, dtype=np.uint16), min_size=2, max_segments=256, depth_abs=0.003)
        check_equal(seeded(rng, shape, dtype=np.uint16), depth_scale=0.000125, min_size=1, depth_abs=0.001, depth_quad=0.004)
    want, _ = check_equal(seeded(rng, (37, 200)), min_size=5)
    assert want[2][0] > 2 and want[2][2] > want[2][1]
    check_equal(seeded(rng, (2 * TH + 1, 2 * TW + 1), density=0.0), min_size=1)                # nothing kept
    check_equal(seeded(rng, (2 * TH + 1, 2 * TW + 1), density=1.0), min_size=1, z_min=1.0, z_max=1.25)
    wide = seeded(rng, (37, 200 + 37))
    view = wide[:, 5:5 + 200]
    assert view.strides[0] > 200 * 4
    check_equal(view, min_size=3)
    wide16 = seeded(rng, (TH + 1, TW + 4), dtype=np.uint16)
    check_equal(wide16[:, 2:2 + TW + 1], min_size=1)


def serpentine(shape):
    """a one-pixel-wide path: along every other row, joined alternately at the right and the left end"""
    img = np.zeros(shape, np.float32)
    img[0::2, :] = 1.0
    for k, v in enumerate(range(1, shape[0], 2)):
        img[v, shape[1] - 1 if k % 2 == 0 else 0] = 1.0
    return img


def comb(shape):
    """a spine along the bottom row and a tooth up every other column"""
    img = np.zeros(shape, np.float32)
    img[:, 0::2] = 1.0
    img[shape[0] - 1, :] = 1.0
    return img


def spiral_path(shape):
    """the pixels of a one-pixel-wide square spiral inwards, one empty pixel between its arms, in walking order"""
    seen = np.zeros(shape, bool)
    inside = lambda v, u: 0 <= v < shape[0] and 0 <= u < shape[1]
    v, u, dv, du = 0, 0, 0, 1
    seen[0, 0] = True
    path = [(0, 0)]
    while True:
        for _ in range(2):              # straight on, or one turn to the right
            ahead, beyond = (v + dv, u + du), (v + 2 * dv, u + 2 * du)
            if inside(*ahead) and not seen[ahead] and not (inside(*beyond) and seen[beyond]):
                break
            dv, du = du, -dv
        else:
            return path
        v, u = ahead
        seen[v, u] = True
        path.append((v, u))


def spiral(shape):
    img = np.zeros(shape, np.float32)
    for v, u in spiral_path(shape):
        img[v, u] = 1.0
    return img


@pytest.mark.parametrize("draw", [serpentine, comb, spiral])
def test_chains_across_tiles(draw):
    shape = (4 * TH + 1, 3 * TW + 1)
    img = draw(shape)
    want, _ = check_equal(img, min_size=1)
    kept = int((img > 0).sum())
    assert want[2] == (1, 1, 1) and want[1][0]["n_pixels"] == kept and want[1][0]["first_pixel"] == 0
    # one link cut in the middle of the chain: a pixel of the component whose removal splits it
    cut = img.copy()
    if draw is comb:
        cut[shape[0] - 1, shape[1] // 2 + 1] = 0.0              # the spine, between two teeth
    elif draw is serpentine:
        cut[2 * TH, shape[1] // 2] = 0.0
    else:
        path = spiral_path(shape)
        cut[path[len(path) // 2]] = 0.0
    want, _ = check_equal(cut, min_size=1)
    assert want[2] == (2, 2, 2) and want[1][0]["n_pixels"] + want[1][1]["n_pixels"] == kept - 1
    check_equal(cut, min_size=1, flags=S.EIGHT)


def test_a_component_that_reaches_a_tile_through_two_neighbours():
    """a ring around the corner where four tiles meet: tile (1, 1) holds two pieces of it that only join through tiles
    (0, 1) and (1, 0); one root, its size counted once"""
    img = np.zeros((2 * TH, 2 * TW), np.float32)
    img[TH - 4, TW - 6:TW + 7] = 1.0
    img[TH + 4, TW - 6:TW + 7] = 1.0
    img[TH - 4:TH + 5, TW - 6] = 1.0
    img[TH - 4:TH + 5, TW + 6] = 1.0
    img[TH + 1, TW + 6] = 0.0            # cut inside tile (1, 1): its two pieces meet only outside it
    want, _ = check_equal(img, min_size=1)
    assert want[2] == (1, 1, 1) and want[1][0]["n_pixels"] == int((img > 0).sum())
    # a U whose two arms hang into the lower tiles from one bar in the upper ones
    img = np.zeros((2 * TH, 2 * TW), np.float32)
    img[2, 3:TW + 20] = 1.0
    img[2:2 * TH, 3] = 1.0
    img[2:2 * TH, TW + 19] = 1.0
    img[2 * TH - 1, 3:TW + 20:2] = 1.0
    want, _ = check_equal(img, min_size=1)
    assert want[2][2] == int((img[2 * TH - 1, 5:TW + 18:2] > 0).sum()) + 1


def test_chessboard_and_threshold_closures():
    img = chessboard((TH + 3, TW + 5))
    kept = int((img > 0).sum())
    want, _ = check_equal(img, min_size=1, max_segments=256)
    assert want[2] == (256, kept, kept)
    want, _ = check_equal(img, min_size=1, flags=S.EIGHT)
    assert want[2] == (1, 1, 1)
    zq = np.float32(1.0078125)
    for q, n in ((zq, 1), (np.nextafter(zq, np.float32(2)), 2)):
        assert check_equal(plateaus(q), depth_abs=0.0078125, min_size=1)[0][2][2] == n
    for q, n in ((np.float32(0.5), 1), (np.nextafter(np.float32(0.5), np.float32(0)), 2)):
        assert check_equal(plateaus(np.float32(2.0)), depth_abs=0.0, depth_quad=q, min_size=1)[0][2][2] == n
        nrm = with_normals(np.full((4, 6), ONE), lambda v, u: (0, 0, 1) if u < 3 else (1, 0, q), lambda v, u: 0.0)
        assert check_equal(np.full((4, 6), ONE), normals=nrm, normal_cos=0.5, min_size=1)[0][2][2] == n
    t = np.float32(0.03)
    img = np.full((3, 5), ONE)
    for cv, smooth in ((t, 15), (np.nextafter(t, ONE), 14), (np.float32(np.nan), 14)):
        nrm = with_normals(img, lambda v, u: (0, 0, 1), lambda v, u: cv if (v, u) == (1, 2) else 0.0)
        assert check_equal(img, normals=nrm, min_size=1)[0][3]["n_smooth"] == smooth
    nrm = with_normals(img, lambda v, u: (0, 0, 1), lambda v, u: 7.0)
    assert check_equal(img, normals=nrm, min_size=1, curvature_threshold=np.inf)[0][2] == (1, 1, 1)


def test_with_normals_across_the_tile_edges():
    rng = np.random.default_rng(242)
    for shape in ((1, 7), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1), (37, 200)):
        img = seeded(rng, shape)
        nrm = seeded_normals(rng, img)
        for flags in (0, S.EIGHT, S.UNORIENTED, S.EIGHT | S.UNORIENTED):
            want, _ = check_equal(img, normals=nrm, min_size=1, max_segments=256, flags=flags)
        if shape == (37, 200):
            assert want[3]["n_attached"] > 50 and want[3]["n_eligible"] < want[3]["n_kept"]
    u16 = seeded(rng, (TH + 5, TW + 9), dtype=np.uint16)
    check_equal(u16, normals=seeded_normals(rng, u16), min_size=2)
    # border pixels on both sides of a tile edge in u and in v, whose only or best smooth neighbour lies in the next tile
    shape = (2 * TH + 2, 2 * TW + 2)
    v, u = np.mgrid[0:shape[0], 0:shape[1]]
    img = (1.0 + 0.001 * u + 0.0015 * v).astype(np.float32)
    border = ((u == TW - 1) | (u == TW) | (v == TH - 1) | (v == TH)) & ((u + v) % 3 != 0)
    nrm = with_normals(img, lambda v, u: (0, 0, -1), lambda v, u: 1.0 if border[v, u] else 0.0)
    for flags in (0, S.EIGHT):
        want, _ = check_equal(img, normals=nrm, min_size=1, flags=flags)
        assert want[3]["n_attached"] > 0
    lone = np.zeros(shape, bool)
    lone[TH - 1, 5], lone[3, TW - 1], lone[TH, 9], lone[7, TW] = True, True, True, True
    gap = img.copy()
    gap[TH - 2, 5] = gap[TH - 1, 4] = gap[TH - 1, 6] = 0.0      # (TH - 1, 5): the only smooth neighbour is (TH, 5), in the next tile
    gap[2, TW - 1] = gap[4, TW - 1] = gap[3, TW - 2] = 0.0      # (3, TW - 1): only (3, TW)
    nrm = with_normals(gap, lambda v, u: (0, 0, -1), lambda v, u: 1.0 if lone[v, u] else 0.0)
    want, _ = check_equal(gap, normals=nrm, min_size=1)
    assert want[3]["n_attached"] == 4 and want[0][TH - 1, 5] == want[0][TH, 5] >= 0 and want[0][3, TW - 1] == want[0][3, TW] >= 0


def test_a_normals_cloud_of_the_wrong_row_count_is_refused():
    import torch
    rng = np.random.default_rng(243)
    img = seeded(rng, (TH + 1, TW + 1))
    rows, curv = seeded_normals(rng, img)
    for bad in ((rows[:-1], curv[:-1]), (np.vstack([rows, rows[:3]]), np.concatenate([curv, curv[:3]])), (rows[:0], curv[:0])):
        labels = np.full(img.shape, 7, np.int32)
        with pytest.raises(_capi.PPFError) as e:
            segment_depth(img, normals=cloud_of(bad), out=labels)
        assert e.value.status == _capi.PPF_ERR_INVALID and (labels == 7).all()
    # the raw entry: info, counts and stats come back zero
    cloud = cloud_of((rows[:-1], curv[:-1]))
    dp, sp = _capi.DepthParams(), _capi.SegmentParams()
    _capi.lib().ppf_default_depth_params(dp)
    _capi.lib().ppf_default_segment_params(sp)
    info = (_capi.SegmentInfo * sp.max_segments)()
    info[0].n_pixels = info[63].n_pixels = 9
    counts = (_capi.C.c_int32 * 3)(9, 9, 9)
    st = _capi.SegmentStats(n_kept=9, n_launches=9)
    labels = np.full(img.shape, 7, np.int32)
    assert _capi.lib().ppf_depth_segments(img.ctypes.data, img.shape[0], img.shape[1], 0, dp, cloud._ptr, sp, labels.ctypes.data, info, counts,
                                          st) == _capi.PPF_ERR_INVALID
    assert list(counts) == [0, 0, 0] and info[0].n_pixels == 0 and info[63].n_pixels == 0 and st.n_kept == 0 and st.n_launches == 0
    assert (labels == 7).all()
    torch.cuda.synchronize()


def blocks(n_side, size):
    """n_side x n_side squares of size x size pixels, one pixel apart"""
    img = np.zeros((n_side * (size + 1), n_side * (size + 1)), np.float32)
    for i in range(n_side):
        for j in range(n_side):
            img[i * (size + 1):i * (size + 1) + size, j * (size + 1):j * (size + 1) + size] = 1.0
    return img


def test_ranking_at_its_capacity():
    img = blocks(17, 2)                       # 289 components of 4 pixels: equal sizes, ranked by their first pixel
    rng = np.random.default_rng(244)
    for k in rng.choice(289, 40, replace=False):          # 40 of them lose a pixel, 3 more lose two
        img[(k // 17) * 3 + 1, (k % 17) * 3 + 1] = 0.0
    for k in (5, 100, 288):
        img[(k // 17) * 3, (k % 17) * 3 + 1] = 0.0
    for kw in (dict(max_segments=256), dict(max_segments=1), dict(max_segments=64, min_size=3), dict(max_segments=256, min_size=4),
               dict(max_segments=256, max_size=3)):
        want, _ = check_equal(img, **dict(dict(min_size=1), **kw))
    want, _ = check_equal(img, min_size=1, max_segments=256)
    assert want[2] == (256, 289, 289)
    firsts = [i["first_pixel"] for i in want[1] if i["n_pixels"] == 4]
    assert firsts == sorted(firsts) and len(firsts) > 200


def test_host_and_device_entries_out_a_side_stream_and_refusals():
    import torch
    rng = np.random.default_rng(245)
    shape = (37, 200)
    img = seeded(rng, shape)
    nrm = seeded_normals(rng, img)
    cloud = cloud_of(nrm)
    prm = dict(min_size=4, flags=S.EIGHT)
    want, _ = check_equal(img, normals=nrm, **prm)
    t = torch.from_numpy(img).cuda()
    got, info, counts, st = segment_depth(t, normals=cloud, params=prm, return_info=True, return_stats=True)
    assert got.is_cuda and got.dtype == torch.int32 and got.cpu().numpy().tobytes() == want[0].tobytes()
    assert info_rows(info) == want[1] and tuple(int(c) for c in counts) == want[2] and {k: st[k] for k in want[3]} == want[3]
    out = torch.full(shape, 7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert segment_depth(t, normals=cloud, params=prm, out=out) is out
    assert out.cpu().numpy().tobytes() == want[0].tobytes()
    wide = torch.from_numpy(np.ascontiguousarray(np.pad(img, ((0, 0), (8, 16)), constant_values=1.0))).cuda()      # a strided tensor
    view = wide[:, 8:8 + shape[1]]
    assert not view.is_contiguous() and segment_depth(view, normals=cloud, params=prm, out=out) is out
    assert out.cpu().numpy().tobytes() == want[0].tobytes()
    u16 = seeded(rng, shape, dtype=np.uint16)
    want16, _ = check_equal(u16, depth_scale=0.000125, min_size=2, depth_abs=0.001)
    got16 = segment_depth(torch.from_numpy(u16).cuda(), depth_scale=0.000125, params=dict(min_size=2, depth_abs=0.001))
    assert got16.cpu().numpy().tobytes() == want16[0].tobytes()
    host_out = np.full(shape, 7, np.int32)
    assert segment_depth(img, normals=cloud, params=prm, out=host_out) is host_out and host_out.tobytes() == want[0].tobytes()
    with pytest.raises(_capi.PPFError):
        segment_depth(img, params=dict(min_sise=3))                         # a misspelt key
    # the label buffer must not overlap the image, and must be what it says
    n = shape[0] * shape[1]
    buf = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    ibuf = buf.view(torch.int32)
    for call in (lambda: segment_depth(buf[:n].view(shape), out=ibuf[n // 2:n // 2 + n].view(shape)),
                 lambda: segment_depth(buf[:n].view(shape), out=ibuf[:n].view(shape)),
                 lambda: segment_depth(t, out=torch.zeros((shape[0], shape[1] + 1), dtype=torch.int32, device="cuda")),
                 lambda: segment_depth(t, out=torch.zeros((shape[0] - 1, shape[1]), dtype=torch.int32, device="cuda")),      # undersized
                 lambda: segment_depth(t, out=torch.zeros(shape, dtype=torch.float32, device="cuda")),
                 lambda: segment_depth(t, out=torch.zeros(shape, dtype=torch.int32))):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID
    assert segment_depth(buf[:n].view(shape), out=ibuf[n:].view(shape)) is not None          # side by side is fine
    torch.cuda.synchronize()


def test_launches_and_waits_do_not_depend_on_the_content():
    rng = np.random.default_rng(246)
    shape = (37, 200)
    imgs = (seeded(rng, shape, 0.3), np.full(shape, ONE), np.zeros(shape, np.float32))
    plain = [segment_depth(img, params=dict(min_size=1), return_stats=True)[1] for img in imgs]
    assert len({st["n_kept"] for st in plain}) == 3
    assert len({(st["n_launches"], st["n_host_syncs"]) for st in plain}) == 1 and plain[0]["n_host_syncs"] == 1
    with_n = [segment_depth(img, normals=cloud_of(seeded_normals(rng, img)), params=dict(min_size=1), return_stats=True)[1] for img in imgs]
    assert len({(st["n_launches"], st["n_host_syncs"]) for st in with_n}) == 1 and with_n[0]["n_host_syncs"] == 1
    assert with_n[0]["n_launches"] > plain[0]["n_launches"]
    # 5 stage kernels + 4 digit passes of 7 launches + 2; a normals cloud adds k_depth_count and a five-launch scan
    assert (plain[0]["n_launches"], with_n[0]["n_launches"]) == (35, 41)
    other = segment_depth(seeded(rng, (2 * TH + 1, 2 * TW + 1)), return_stats=True)[1]          # nor on the image's size
    assert other["n_launches"] == plain[0]["n_launches"]


def test_repeated_and_concurrent_calls():
    rng = np.random.default_rng(247)
    imgs = [seeded(rng, (60, 300)), seeded(rng, (60, 300), 0.6)]
    nrms = [seeded_normals(rng, img) for img in imgs]
    clouds = [cloud_of(n) for n in nrms]
    want = [check_equal(img, normals=n, min_size=3)[0][0].tobytes() for img, n in zip(imgs, nrms)]
    got = [None, None]

    def work(j):
        got[j] = [segment_depth(imgs[j], normals=clouds[j], params=dict(min_size=3)).tobytes() for _ in range(3)]
    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(g == want[j] for j in range(2) for g in got[j])


def words(a):
    return int(np.ascontiguousarray(a).view(np.uint32).astype(np.uint64).sum())


def test_reference_window_end_to_end_and_the_cpp_demo(tmp_path):
    import torch
    win, filtered, shifted, nrm = reference_window()
    want = S.segments(filtered, normals=nrm)
    assert want[2][0] >= 2
    t = torch.from_numpy(win).cuda()
    f = filter_depth(t)
    cloud = DeviceCloud.from_depth(f, shifted, fp64=True, normals={})
    labels, info, counts, st = segment_depth(f, normals=cloud, return_info=True, return_stats=True)
    assert labels.cpu().numpy().tobytes() == want[0].tobytes() and info_rows(info) == want[1] and tuple(int(c) for c in counts) == want[2]
    assert {k: st[k] for k in want[3]} == want[3]
    K = np.array([[shifted[0], 0, shifted[2]], [0, shifted[1], shifted[3]], [0, 0, 1]], np.float64)
    cp = CloudProcessor(None, win, [], [], [], 0.05, 0.05)
    cp.FilterDepth()
    cp.Deprojection(K, fp64=True, normals={})
    got = cp.ProposeSegments()
    assert got.tobytes() == want[0].tobytes() and cp.segment_labels is got
    assert cp.boxes == [i["box_xywh"] for i in want[1]] and info_rows(cp.segment_info) == want[1]
    assert {k: cp.segment_stats[k] for k in want[3]} == want[3]
    plain = S.segments(filtered, min_size=50, flags=S.EIGHT)
    cp.RemovePlanes(max_planes=1)                     # the scene is no longer the image's normals cloud: depth alone decides
    cp.ProposeSegments(dict(min_size=50, flags=_capi.PPF_SEGMENT_EIGHT))
    assert cp.segment_labels.tobytes() == plain[0].tobytes() and cp.boxes == [i["box_xywh"] for i in plain[1]]
    # the demo: filter -> normals -> segments on the raw float32 file
    exe = str(tmp_path / "depth_segments_demo")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "depth_segments_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    (tmp_path / "depth.f32").write_bytes(win.tobytes())
    for prm in (dict(), dict(depth_abs=0.004, depth_quad=0.001, normal_cos=0.9, curvature_threshold=0.05, min_size=30, max_size=20000,
                             max_segments=9, flags=3)):
        full = dict(S.DEFAULTS, **prm)
        args = [repr(float(full[k])) for k in ("depth_abs", "depth_quad", "normal_cos", "curvature_threshold")] + \
               [str(full[k]) for k in ("min_size", "max_size", "max_segments", "flags")]
        r = subprocess.run([exe, str(tmp_path / "depth.f32"), str(win.shape[0]), str(win.shape[1])] + [repr(float(v)) for v in shifted] + args,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        labels, info, counts, st = segment_depth(f, normals=cloud, params=prm, return_info=True, return_stats=True)
        lines = [f"kept {st['n_kept']} eligible {st['n_eligible']} smooth {st['n_smooth']} attached {st['n_attached']}",
                 f"segments {counts[0]} valid {counts[1]} components {counts[2]}"]
        for k, row in enumerate(info[:5]):
            b = row["box_xywh"]
            lines.append(f"segment {k} pixels {row['n_pixels']} border {row['n_border']} first {row['first_pixel']} box {b[0]} {b[1]} {b[2]} {b[3]}")
        lines.append(f"label checksum {words(labels.cpu().numpy())}")
        assert r.stdout.strip().splitlines() == lines
        assert counts[0] >= 2
