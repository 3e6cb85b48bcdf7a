"""ppf_depth_edges on the device against the numpy oracle (tests/depth_edges_oracle.py): the mask byte for byte, every count
of the stats and the edge cloud's rows and curvatures byte for byte.  Shapes across the kernel's tile edges in both directions,
seeded content with holes and non-finite values, both formats, a pitched input, every max_gap with holes wider than the halo
and gaps that run into the image border, partners max_gap + 1 away in the next tile, nothing kept and everything kept, the z
range, the cloud with and without normals for every select, the host and the device entry, launches that do not depend on the
content, concurrent calls, the C++ demo, and the reference window through filter -> normals -> edges -> match in S2B mode."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import depth_edges_oracle as E
import depth_normals_oracle as N
from test_depth_edges_oracle import seeded_normals
from test_depth_filter_oracle import seeded
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, depth_edges, filter_depth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
TW, TH = 64, 16            # the tile of k_depth_edges (ppf_edge_kernels.h)
DEPTH_KEYS = ("depth_scale", "z_min", "z_max", "fp64")
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 3), (TH, TW), (TH - 1, TW - 1), (TH + 1, TW + 1), (TH, TW + 1), (TH + 1, TW), (37, 200)]
ONE = np.float32(1.0)
INTR = (150.0, 151.0, 79.5, 59.25)
LAUNCHES = {(False, False): (1, 1), (True, False): (7, 1), (False, True): (7, 2), (True, True): (13, 2)}   # (normals, cloud)


def cloud_of(normals):
    rows, curv = normals
    return DeviceCloud.upload(rows, curvature=curv) if len(rows) else DeviceCloud.upload(np.zeros((0, 6), np.float32))


def check_equal(img, intr=None, normals=None, cloud=None, **kw):
    """the device's mask, counts and edge cloud are the oracle's; returns the oracle's result and the device's stats"""
    dk = {k: v for k, v in kw.items() if k in DEPTH_KEYS}
    ek = {k: v for k, v in kw.items() if k not in DEPTH_KEYS}
    cloud = (intr is not None or normals is not None) if cloud is None else cloud
    want = E.edges(img, intr if cloud else None, normals=normals, **kw)
    nrm = cloud_of(normals) if normals is not None else None
    got = depth_edges(img, intr, normals=nrm, params=ek, cloud=cloud, return_stats=True, **dk)
    mask, st = got[0], got[-1]
    assert mask.dtype == np.uint8 and mask.shape == want[0].shape
    if mask.tobytes() != want[0].tobytes():
        bad = np.argwhere(mask != want[0])
        v, u = bad[0]
        raise AssertionError(f"{img.shape} {kw}: {len(bad)} mask bytes differ, first ({v}, {u}): {mask[v, u]} against {want[0][v, u]}")
    ws = dict(want[2])
    if not cloud:
        ws["n_rows"] = 0
        if normals is not None:          # the oracle makes a cloud whenever it has normals; the counts are the same
            assert want[2]["n_rows"] == want[2]["n_selected"] - want[2]["n_no_normal"]
    assert {k: st[k] for k in E.STAT_KEYS} == ws, (img.shape, kw, st, ws)
    assert (st["n_launches"], st["n_host_syncs"]) == LAUNCHES[(normals is not None, cloud)], (st, normals is not None, cloud)
    if cloud:
        rows, curv = got[1].download()
        assert len(got[1]) == want[2]["n_rows"]
        assert rows.tobytes() == want[1][0].tobytes() and curv.tobytes() == want[1][1].tobytes(), (img.shape, kw)
    return want, st


def test_shapes_across_the_tile_edges_both_formats_and_a_pitched_view():
    rng = np.random.default_rng(351)
    for shape in SHAPES:
        check_equal(seeded(rng, shape))
        check_equal(seeded(rng, shape, density=0.5), INTR, max_gap=1)
        check_equal(seeded(rng, shape, dtype=np.uint16), depth_abs=0.003)
        check_equal(seeded(rng, shape, dtype=np.uint16), INTR, depth_scale=0.000125, depth_abs=0.001, depth_quad=0.004, fp64=True)
    want, _ = check_equal(seeded(rng, (37, 200)))
    assert want[2]["n_occluding"] > 50 and want[2]["n_occluded"] > 50 and want[2]["n_boundary"] > 50
    wide = seeded(rng, (37, 200 + 37))
    view = wide[:, 5:5 + 200]
    assert view.strides[0] > 200 * 4
    check_equal(view, INTR)
    wide16 = seeded(rng, (TH + 1, TW + 4), dtype=np.uint16)
    check_equal(wide16[:, 2:2 + TW + 1])


def test_density_0_density_1_and_the_z_range():
    rng = np.random.default_rng(352)
    shape = (2 * TH + 1, 2 * TW + 1)
    want, _ = check_equal(seeded(rng, shape, density=0.0), INTR)               # nothing kept
    assert want[2]["n_kept"] == 0 and want[2]["n_rows"] == 0
    want, _ = check_equal(seeded(rng, shape, density=1.0), INTR)
    assert want[2]["n_kept"] == shape[0] * shape[1] and want[2]["n_boundary"] == 0 and want[2]["n_occluding"] > 0
    img = seeded(rng, shape, density=1.0)
    want, _ = check_equal(img, INTR, z_min=1.0, z_max=1.25)                   # the cut makes holes: boundaries appear
    assert 0 < want[2]["n_kept"] < img.size and want[2]["n_boundary"] > 0
    check_equal(img, z_min=1.2)
    check_equal(seeded(rng, shape, dtype=np.uint16, density=1.0), INTR, z_max=1.1)


@pytest.mark.parametrize("max_gap", range(0, 9))
def test_every_max_gap_with_wide_holes_and_gaps_into_the_border(max_gap):
    rng = np.random.default_rng(360 + max_gap)
    shape = (2 * TH + 3, 2 * TW + 5)
    img = seeded(rng, shape, density=0.45)
    img[:, TW - 3:TW + 9] = 0                     # a band wider than the widest halo, across a tile edge
    img[TH - 2:TH + 10, :] = np.nan
    img[:, -(max_gap + 1):] = 0                   # a gap that ends at the image border
    img[:max_gap, :] = 0
    want, _ = check_equal(img, INTR, max_gap=max_gap)
    assert want[2]["n_boundary"] > 0
    check_equal(seeded(rng, (TH + 2, TW + 2), density=0.7), max_gap=max_gap, depth_quad=0.01)


@pytest.mark.parametrize("max_gap", [0, 2, 8])
def test_a_partner_max_gap_plus_1_away_in_the_next_tile(max_gap):
    """an edge pixel on a tile's last row and last column whose partner lies max_gap + 1 further, across the hole, in the
    next tile -- straight and diagonal -- and one pixel beyond reach"""
    g = max_gap
    shape = (2 * TH + 12, 2 * TW + 12)
    img = np.zeros(shape, np.float32)
    near, far = np.float32(1.0), np.float32(1.5)
    img[5, TW - 1], img[5, TW + g] = near, far                         # along the row, across the column edge
    img[TH - 1, 7], img[TH + g, 7] = near, far                         # along the column, across the row edge
    img[TH - 1, TW - 1], img[TH + g, TW + g] = near, far               # the diagonal, across the corner
    img[TH + g + 12, TW - 1], img[TH + g + 12, TW + g + 1] = near, far # one too far: both are boundaries
    want, _ = check_equal(img, max_gap=g)
    m = want[0]
    assert m[5, TW - 1] & E.OCCLUDING and m[5, TW + g] & E.OCCLUDED
    assert m[TH - 1, 7] & E.OCCLUDING and m[TH + g, 7] & E.OCCLUDED
    assert m[TH - 1, TW - 1] & E.OCCLUDING and m[TH + g, TW + g] & E.OCCLUDED
    assert m[TH + g + 12, TW - 1] == E.BOUNDARY and m[TH + g + 12, TW + g + 1] == E.BOUNDARY
    solid = np.full(shape, near)
    solid[:, TW:TW + g] = 0
    solid[:, TW + g:] = far
    solid[TH:TH + g, :] = 0
    want, _ = check_equal(solid, INTR, max_gap=g)
    assert want[2]["n_occluding"] >= shape[0] - g and (g > 0 or want[2]["n_boundary"] == 0)


def test_the_cloud_with_normals_for_every_select():
    rng = np.random.default_rng(353)
    img = seeded(rng, (21, 131), density=0.7)
    intr = (120.0, 119.0, 64.3, 10.1)
    real = DeviceCloud.from_depth(img, intr, normals=dict(radius=1, min_neighbours=6))   # the device's own normals cloud for this image
    rows, curv = real.download()
    assert rows.shape[0] == int(N.keep_mask(img).sum()) and not np.isfinite(rows[:, 3:6]).all() and (curv > 0.03).any()
    index = np.full(img.shape, -1)
    index[N.keep_mask(img)] = np.arange(rows.shape[0])
    for select in range(1, 16):
        mask, edge, st = depth_edges(img, normals=real, params=dict(select=select), cloud=True, return_stats=True)
        want = E.edges(img, normals=(rows, curv), select=select)
        assert mask.tobytes() == want[0].tobytes() and {k: st[k] for k in E.STAT_KEYS} == want[2], select
        take = index[(mask & select) != 0]
        take = take[np.isfinite(rows[take, 3:6]).all(axis=1)]
        got_rows, got_curv = edge.download()
        assert got_rows.tobytes() == rows[take].tobytes() and got_curv.tobytes() == curv[take].tobytes(), select
        assert st["n_rows"] == len(take) == st["n_selected"] - st["n_no_normal"]
    assert st["n_no_normal"] > 0
    # seeded normals with NaN rows and NaN curvatures, across the tile edges; the mask alone with normals
    for shape in ((1, 7), (TH + 1, TW + 1), (37, 200)):
        img = seeded(rng, shape, density=0.6)
        nrm = seeded_normals(rng, img)
        check_equal(img, normals=nrm)
        check_equal(img, normals=nrm, cloud=False, select=E.CURVATURE | E.OCCLUDED, curvature_threshold=0.01)
    u16 = seeded(rng, (TH + 5, TW + 9), dtype=np.uint16)
    check_equal(u16, normals=seeded_normals(rng, u16), curvature_threshold=np.inf)
    pair, edge = DeviceCloud.from_depth(img, intr, normals={}, edges={})
    want = depth_edges(img, normals=pair, cloud=True)[1]
    assert edge.download()[0].tobytes() == want.download()[0].tobytes() and len(edge) > 0


def test_the_cloud_without_normals_is_the_depth_clouds_rows_and_an_empty_selection_is_an_empty_cloud():
    rng = np.random.default_rng(354)
    img = seeded(rng, (37, 200), density=0.8)
    for fp64 in (False, True):
        full = DeviceCloud.from_depth(img, INTR, fp64=fp64).download()[0]
        index = np.full(img.shape, -1)
        index[N.keep_mask(img)] = np.arange(full.shape[0])
        for select in (E.OCCLUDING, E.OCCLUDED | E.BOUNDARY, 15):
            mask, edge, st = depth_edges(img, INTR, fp64=fp64, params=dict(select=select), cloud=True, return_stats=True)
            rows, curv = edge.download()
            assert rows.tobytes() == full[index[(mask & select) != 0]].tobytes() and not curv.any() and st["n_rows"] == len(rows) > 0
        check_equal(img, INTR, fp64=fp64)
    flat = np.full((TH + 3, TW + 3), ONE)
    want, st = check_equal(flat, INTR)
    assert st["n_rows"] == 0 and st["n_edge"] == 0
    mask, edge = depth_edges(flat, INTR, params=dict(select=E.CURVATURE), cloud=True)       # no normals: the bit is never set
    assert len(edge) == 0 and edge.download()[0].shape == (0, 6)
    want, st = check_equal(flat, normals=(np.tile(np.array([[0, 0, 1, 0, 0, -1]], np.float32), (flat.size, 1)), np.zeros(flat.size, np.float32)))
    assert st["n_rows"] == 0


def test_a_normals_cloud_of_the_wrong_row_count_is_refused():
    import torch
    rng = np.random.default_rng(355)
    img = seeded(rng, (TH + 1, TW + 1))
    rows, curv = seeded_normals(rng, img)
    for bad in ((rows[:-1], curv[:-1]), (np.vstack([rows, rows[:3]]), np.concatenate([curv, curv[:3]])), (rows[:0], curv[:0])):
        for cloud in (False, True):
            mask = np.full(img.shape, 7, np.uint8)
            with pytest.raises(_capi.PPFError) as e:
                depth_edges(img, normals=cloud_of(bad), out=mask, cloud=cloud)
            assert e.value.status == _capi.PPF_ERR_INVALID and (mask == 7).all() and "rows" in str(e.value)
    # the raw entry: *out_cloud NULL and the stats zero
    nrm = cloud_of((rows[:-1], curv[:-1]))
    dp, ep = _capi.DepthParams(), _capi.DepthEdgeParams()
    _capi.lib().ppf_default_depth_params(dp)
    _capi.lib().ppf_default_depth_edge_params(ep)
    st = _capi.DepthEdgeStats(n_kept=9, n_launches=9)
    found = C.c_void_p(0x5A5A)
    mask = np.full(img.shape, 7, np.uint8)
    assert _capi.lib().ppf_depth_edges(img.ctypes.data, img.shape[0], img.shape[1], 0, None, dp, nrm._ptr, ep, mask.ctypes.data, C.byref(found),
                                       st) == _capi.PPF_ERR_INVALID
    assert found.value is None and st.n_kept == 0 and st.n_launches == 0 and (mask == 7).all()
    torch.cuda.synchronize()


def test_host_and_device_entries_out_a_side_stream_and_refusals():
    import torch
    rng = np.random.default_rng(356)
    shape = (37, 200)
    img = seeded(rng, shape, density=0.7)
    nrm = seeded_normals(rng, img)
    cloud = cloud_of(nrm)
    prm = dict(max_gap=3, depth_abs=0.01)
    want, _ = check_equal(img, normals=nrm, **prm)
    t = torch.from_numpy(img).cuda()
    got, edge, st = depth_edges(t, normals=cloud, params=prm, cloud=True, return_stats=True)
    assert got.is_cuda and got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want[0].tobytes()
    assert {k: st[k] for k in E.STAT_KEYS} == want[2] and (st["n_launches"], st["n_host_syncs"]) == LAUNCHES[(True, True)]
    assert edge.download()[0].tobytes() == want[1][0].tobytes() and edge.download()[1].tobytes() == want[1][1].tobytes()
    plain = E.edges(img, INTR, **prm)
    for with_cloud in (False, True):                                        # the device entry's other two modes
        res = depth_edges(t, INTR, params=prm, cloud=with_cloud, return_stats=True)
        assert res[0].cpu().numpy().tobytes() == plain[0].tobytes()
        assert (res[-1]["n_launches"], res[-1]["n_host_syncs"]) == LAUNCHES[(False, with_cloud)]
        if with_cloud:
            assert res[1].download()[0].tobytes() == plain[1][0].tobytes() and res[-1]["n_rows"] == plain[2]["n_rows"]
    res = depth_edges(t, normals=cloud, params=prm, return_stats=True)
    assert res[0].cpu().numpy().tobytes() == want[0].tobytes() and (res[1]["n_launches"], res[1]["n_host_syncs"]) == LAUNCHES[(True, False)]
    out = torch.full(shape, 7, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert depth_edges(t, normals=cloud, params=prm, out=out) is out
    assert out.cpu().numpy().tobytes() == want[0].tobytes()
    wide = torch.from_numpy(np.ascontiguousarray(np.pad(img, ((0, 0), (8, 16)), constant_values=1.0))).cuda()      # a strided tensor
    view = wide[:, 8:8 + shape[1]]
    assert not view.is_contiguous() and depth_edges(view, normals=cloud, params=prm, out=out) is out
    assert out.cpu().numpy().tobytes() == want[0].tobytes()
    u16 = seeded(rng, shape, dtype=np.uint16)
    want16 = E.edges(u16, INTR, depth_scale=0.000125, depth_abs=0.001)
    got16, edge16 = depth_edges(torch.from_numpy(u16).cuda(), INTR, depth_scale=0.000125, params=dict(depth_abs=0.001), cloud=True)
    assert got16.cpu().numpy().tobytes() == want16[0].tobytes() and edge16.download()[0].tobytes() == want16[1][0].tobytes()
    host_out = np.full(shape, 7, np.uint8)
    assert depth_edges(img, normals=cloud, params=prm, out=host_out) is host_out and host_out.tobytes() == want[0].tobytes()
    # the cloud alone: edges NULL, on both entries
    dp, ep = _capi.DepthParams(), _capi.DepthEdgeParams()
    _capi.lib().ppf_default_depth_params(dp)
    _capi.lib().ppf_default_depth_edge_params(ep)
    ep.max_gap, ep.depth_abs = 3, 0.01
    it = (C.c_double * 4)(*INTR)
    for nptr, ref in ((None, plain), (cloud._ptr, want)):
        found, st = C.c_void_p(), _capi.DepthEdgeStats()
        _capi.check(_capi.lib().ppf_depth_edges(img.ctypes.data, shape[0], shape[1], 0, it, dp, nptr, ep, None, C.byref(found), st))
        assert DeviceCloud(found).download()[0].tobytes() == ref[1][0].tobytes() and st.n_rows == ref[2]["n_rows"]
        found = C.c_void_p()
        _capi.check(_capi.lib().ppf_depth_edges_device(C.c_void_p(t.data_ptr()), shape[0], shape[1], 0, it, dp, nptr, ep, None, None, C.byref(found), st))
        assert DeviceCloud(found).download()[0].tobytes() == ref[1][0].tobytes() and st.n_edge == ref[2]["n_edge"]
    # the mask buffer must not overlap the image, and must be what it says
    n = shape[0] * shape[1]
    buf = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    bbuf = buf.view(torch.uint8)
    for call in (lambda: depth_edges(buf[:n].view(shape), out=bbuf[2 * n:3 * n].view(shape)),
                 lambda: depth_edges(buf[:n].view(shape), out=bbuf[:n].view(shape)),
                 lambda: depth_edges(t, out=torch.zeros((shape[0], shape[1] + 1), dtype=torch.uint8, device="cuda")),
                 lambda: depth_edges(t, out=torch.zeros((shape[0] - 1, shape[1]), dtype=torch.uint8, device="cuda")),      # undersized
                 lambda: depth_edges(t, out=torch.zeros(shape, dtype=torch.float32, device="cuda")),
                 lambda: depth_edges(t, out=torch.zeros(shape, dtype=torch.uint8))):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID
    assert depth_edges(buf[:n].view(shape), out=bbuf[4 * n:5 * n].view(shape)) is not None          # side by side is fine
    torch.cuda.synchronize()


def test_launches_and_waits_do_not_depend_on_the_content():
    rng = np.random.default_rng(357)
    shape = (37, 200)
    imgs = (seeded(rng, shape, 0.3), np.full(shape, ONE), np.zeros(shape, np.float32), seeded(rng, (2 * TH + 1, 2 * TW + 1)))
    for with_normals in (False, True):
        for with_cloud in (False, True):
            seen = []
            for img in imgs:
                nrm = cloud_of(seeded_normals(rng, img)) if with_normals else None
                st = depth_edges(img, INTR, normals=nrm, cloud=with_cloud, return_stats=True)[-1]
                seen.append((st["n_launches"], st["n_host_syncs"]))
            assert set(seen) == {LAUNCHES[(with_normals, with_cloud)]}, (with_normals, with_cloud, seen)


def test_repeated_and_concurrent_calls():
    rng = np.random.default_rng(358)
    imgs = [seeded(rng, (60, 300)), seeded(rng, (60, 300), 0.6)]
    nrms = [seeded_normals(rng, img) for img in imgs]
    clouds = [cloud_of(n) for n in nrms]
    want = [check_equal(img, normals=n)[0] for img, n in zip(imgs, nrms)]
    got = [None, None]

    def work(j):
        got[j] = []
        for _ in range(3):
            mask, edge = depth_edges(imgs[j], normals=clouds[j], cloud=True)
            got[j].append((mask.tobytes(), edge.download()[0].tobytes()))
    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(g == (want[j][0].tobytes(), want[j][1][0].tobytes()) for j in range(2) for g in got[j])


def words(*arrays):
    return sum(int(np.ascontiguousarray(a).view(np.uint32).astype(np.uint64).sum()) for a in arrays) % (1 << 64)


def test_reference_window_chain_in_s2b_mode_and_the_cpp_demo(tmp_path, bottle):
    """filter -> normals -> edges -> ppf_match_clouds with the edge cloud on the reference's own frame: the chain runs and
    returns poses (no pose value is asserted); then the demo on the raw window against the Python calls"""
    import torch
    from test_depth_segments_oracle import reference_window
    win, filtered, shifted, nrm = reference_window()
    want = E.edges(filtered, normals=nrm)
    t = torch.from_numpy(win).cuda()
    f = filter_depth(t)
    scene, edge = DeviceCloud.from_depth(f, shifted, fp64=True, normals={}, edges={})
    mask, edge2, st = depth_edges(f, normals=scene, cloud=True, return_stats=True)
    assert mask.cpu().numpy().tobytes() == want[0].tobytes() and {k: st[k] for k in E.STAT_KEYS} == want[2]
    assert edge.download()[0].tobytes() == edge2.download()[0].tobytes() == want[1][0].tobytes()
    assert st["n_occluding"] > 100 and len(edge) > 100
    K = np.array([[shifted[0], 0, shifted[2]], [0, shifted[1], shifted[3]], [0, 0, 1]], np.float64)
    cp = CloudProcessor(None, win, [], [], [], 0.025, 0.05)
    cp.FilterDepth()
    cp.Deprojection(K, fp64=True, normals={})
    got = cp.EdgeExtractionDepth()
    assert cp.objects_edges[-1] is got and got.download()[0].tobytes() == want[1][0].tobytes()
    assert cp.depth_edge_mask.tobytes() == want[0].tobytes() and {k: cp.depth_edge_stats[k] for k in E.STAT_KEYS} == want[2]
    cp.LoadSingleModel(bottle, "bottle")
    cp.TrainDetector(0.025, 0.05)
    det = cp.detectors[0]
    mp = det._params(0.05, 0.05, False)
    cap = len(cp.scene) + 8
    out = (_capi.Pose * cap)()
    n = C.c_int(0)
    _capi.check(_capi.lib().ppf_match_clouds(det._model.ptr, cp.scene._ptr, got._ptr, C.byref(mp), out, cap, C.byref(n)))
    assert n.value >= 1 and out[0].num_votes > 0
    # the demo: the depth alone, then with its normals, on the raw float32 file
    exe = str(tmp_path / "depth_edges_demo")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "depth_edges_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    (tmp_path / "depth.f32").write_bytes(win.tobytes())
    raw_scene = DeviceCloud.from_depth(win, shifted, fp64=True, normals={})
    for prm in (dict(), dict(depth_abs=0.01, depth_quad=0.002, max_gap=4, curvature_threshold=0.05, select=9)):
        full = dict(E.DEFAULTS, **prm)
        args = [repr(float(full["depth_abs"])), repr(float(full["depth_quad"])), str(full["max_gap"]), repr(float(full["curvature_threshold"])),
                str(full["select"])]
        r = subprocess.run([exe, str(tmp_path / "depth.f32"), str(win.shape[0]), str(win.shape[1])] + [repr(float(v)) for v in shifted] + args,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = []
        for name, nrm_cloud in (("depth", None), ("normals", raw_scene)):
            m, e, s = depth_edges(win, shifted, fp64=True, normals=nrm_cloud, params=prm, cloud=True, return_stats=True)
            rows, curv = e.download()
            lines.append(f"{name} kept {s['n_kept']} occluding {s['n_occluding']} occluded {s['n_occluded']} boundary {s['n_boundary']} "
                         f"curvature {s['n_curvature']} edge {s['n_edge']} selected {s['n_selected']} no_normal {s['n_no_normal']} rows {len(e)} "
                         f"launches {s['n_launches']} waits {s['n_host_syncs']} mask {int(m.astype(np.uint64).sum())} cloud {words(rows, curv)}")
        assert r.stdout.strip().splitlines() == lines
