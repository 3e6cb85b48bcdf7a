"""ppf_depth_volume on the device against tests/depth_volume_oracle.py, byte for byte: the voxels (ppf_depth_volume_read), the
raycast depth and normal images, the extracted rows and every count, at the smallest volumes that reach each path of the
kernels -- odd nx (the element accesses and the one-voxel last lane), even nx (the 16-byte pairs), tiles and bricks cut in
every axis -- for both formats and entries, pitched and misaligned rows, spoiled pixels, poses that leave part of the volume
behind the camera or outside the image, the weight cap, both ends of ray_step, min_weight 2, determinism, two threads, the
pool guard, the refusals of the device entries, and the wrappers: DepthFusion, CloudProcessor.FuseVolume and the loop scan ->
train -> match.  No test provokes a failing launch."""
import ctypes as C
import threading

import numpy as np
import pytest

import depth_motion_oracle as MO
import depth_volume_cases as VC
import depth_volume_oracle as O
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import lib
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DepthFusion, DepthOdometry, DepthVolume, DeviceCloud, _mat44_mul
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector, Pose3D

pytestmark = pytest.mark.gpu
cases = O.cases
F32 = np.float32
DIMS = [(1, 1, 1), (2, 3, 5), (7, 5, 3), (33, 9, 6), (8, 8, 8)]
IMAGES = [(24, 40), (25, 41)]
RAY_SHAPES = [(1, 1), (17, 33), (60, 80)]


def make(vp):
    return DepthVolume(vp["dims"], vp["voxel"], vp["origin"], vp["trunc"], vp.get("max_weight", 64)), O.Volume(**vp)


def same_voxels(dv, ov, what=""):
    d, w = dv.read()
    assert w.tobytes() == ov.w.tobytes(), (what, "weights", int((w != ov.w).sum()))
    assert d.tobytes() == ov.d.tobytes(), (what, "distances", int((d.view(np.int32) != ov.d.view(np.int32)).sum()))


def integrate_both(dv, ov, img, intr, pose, what="", **kw):
    st = dv.integrate(img, intr, pose, return_stats=True, **kw)
    host = img.cpu().numpy() if type(img).__module__.startswith("torch") else np.asarray(img)
    n = O.integrate(ov, host, intr, pose, **kw)
    assert (st["n_updated"], st["n_launches"], st["n_host_syncs"]) == (n, 1, 1), (what, st, n)
    same_voxels(dv, ov, what)
    return n


def ray_params(vp, **kw):
    z1 = vp["origin"][2] + vp["dims"][2] * vp["voxel"]
    return dict(dict(z_near=max(vp["origin"][2] - 0.1, 0.05), z_far=z1 + 0.1), **kw)


def raycast_both(dv, ov, shape, intr, pose, rp, what="", out=None):
    got = dv.raycast(shape, intr, pose, params=rp, out=out, return_normals=True, return_stats=True)
    depth, normals, st = got
    if out is not None:
        depth, normals = depth.cpu().numpy(), normals.cpu().numpy()
    wd, wn, wst = O.raycast(ov, shape, intr, pose, normals=True, **rp)
    assert depth.tobytes() == wd.tobytes(), (what, "depth", int((depth.view(np.int32) != wd.view(np.int32)).sum()))
    assert normals.tobytes() == wn.tobytes(), (what, "normals", int((normals.view(np.int32) != wn.view(np.int32)).sum()))
    assert {k: st[k] for k in wst} == wst, (what, st, wst)
    plain = dv.raycast(shape, intr, pose, params=rp)      # without the normals image: the same depth
    assert plain.tobytes() == wd.tobytes(), what
    return wst


def extract_both(dv, ov, min_weight=1, what=""):
    cloud, st = dv.extract(dict(min_weight=min_weight), return_stats=True)
    rows, curv = cloud.download()
    want, wst = O.extract(ov, min_weight)
    assert {k: st[k] for k in wst} == wst, (what, st, wst)
    assert rows.shape == want.shape and rows.tobytes() == want.tobytes(), what
    assert not curv.any()
    return wst


def check_box(dims, image=(24, 40), dtype=F32, n_frames=3, max_weight=64, ray_shape=(17, 33), ray_step=0.5, min_weight=1, spoil=False,
              pitch=None):
    """a volume of `dims` filled from n_frames posed images, then raycast and extracted; everything against the oracle.
    Returns the counts, so that callers can see what a case reached."""
    vp = VC.box_volume(dims, max_weight=max_weight)
    dv, ov = make(vp)
    kinds = ["identity", "moved", "behind", "aside", "moved"]
    updated = []
    for f in range(n_frames):
        img, intr = VC.box_frame(vp, image[0], image[1], seed=f, dtype=dtype)
        if spoil and dtype == F32:
            img = cases.spoiled(img, f)
        if pitch is not None:
            img = cases.pitched(img, *pitch)
        pose = VC.box_pose(vp, kinds[f % len(kinds)], seed=f)
        updated.append(integrate_both(dv, ov, img, intr, pose, what=f"{dims} frame {f}", z_min=0.2, z_max=3.0))
    assert dv.info()["integrations"] == n_frames
    rintr = (ray_shape[1] * 1.3, ray_shape[1] * 1.25, (ray_shape[1] - 1) / 2.0 + 0.3, (ray_shape[0] - 1) / 2.0)
    rp = ray_params(vp, ray_step=ray_step, min_weight=min_weight)
    rst = raycast_both(dv, ov, ray_shape, rintr, VC.box_pose(vp, "moved", seed=9), rp, what=f"{dims} raycast")
    xst = extract_both(dv, ov, min_weight, what=f"{dims} extract")
    return updated, rst, xst


@pytest.mark.parametrize("dims", DIMS, ids=[str(d) for d in DIMS])
@pytest.mark.parametrize("image", IMAGES, ids=[f"{r}x{c}" for r, c in IMAGES])
def test_volume_bytes_equal_the_oracle(dims, image):
    updated, rst, xst = check_box(dims, image, n_frames=4)
    assert updated[0] > 0
    if min(dims) >= 3:
        assert updated[2] < updated[0]   # "behind": part of the volume is skipped
    if dims in ((33, 9, 6), (8, 8, 8)):
        assert rst["n_hits"] > 0 and rst["n_interpolated"] > 0 and xst["n_rows"] > 0 and xst["n_crossings"] > xst["n_rows"]


@pytest.mark.parametrize("ray_shape", RAY_SHAPES, ids=[f"{r}x{c}" for r, c in RAY_SHAPES])
@pytest.mark.parametrize("ray_step,min_weight", [(0.5, 1), (1.0, 1), (0.25, 2)])
def test_raycast_shapes_steps_and_weights(ray_shape, ray_step, min_weight):
    _, rst, xst = check_box((33, 9, 6), n_frames=3, ray_shape=ray_shape, ray_step=ray_step, min_weight=min_weight)
    if ray_shape != (1, 1):
        assert rst["n_hits"] > 0
    assert xst["n_crossings"] > 0


def test_uint16_pitched_misaligned_and_spoiled_images():
    check_box((7, 5, 3), (25, 41), dtype=np.uint16)
    check_box((8, 8, 8), (25, 41), dtype=np.uint16, pitch=(3, 1))      # rows 44 elements apart, one element into the buffer
    check_box((8, 8, 8), (24, 40), pitch=(5, 3))
    check_box((33, 9, 6), (24, 40), spoil=True)
    # a pitched image gives the volume of the packed one
    vp = VC.box_volume((8, 8, 8))
    img, intr = VC.box_frame(vp, 24, 40, seed=1)
    a, b = make(vp)[0], make(vp)[0]
    a.integrate(img, intr, np.eye(4))
    b.integrate(cases.pitched(img, 7, 2), intr, np.eye(4))
    assert a.read()[0].tobytes() == b.read()[0].tobytes() and a.read()[1].tobytes() == b.read()[1].tobytes()


@pytest.mark.parametrize("dtype", [F32, np.uint16], ids=["f32", "u16"])
def test_a_z_range_that_cuts_the_surface(dtype):
    """z_min and z_max through the middle of the surface: each leaves out its own part of the pixels, so fewer voxels are
    updated than without a range, the two cuts give different volumes, and each is the oracle's bytes"""
    vp = VC.box_volume((33, 9, 6))
    zc = vp["origin"][2] + 2.5 * vp["voxel"]
    img, intr = VC.box_frame(vp, 24, 40, seed=1, dtype=dtype)
    z = O.metres(img)
    assert z.min() < zc - 0.005 and z.max() > zc + 0.005
    counts, volumes = {}, {}
    for name, kw in (("all", dict()), ("near", dict(z_max=zc)), ("far", dict(z_min=zc)), ("band", dict(z_min=zc - 0.004, z_max=zc + 0.004))):
        dv, ov = make(vp)
        counts[name] = integrate_both(dv, ov, img, intr, np.eye(4), what=f"z range {name}", **kw)
        volumes[name] = ov.records().tobytes()
    assert 0 < counts["near"] < counts["all"] and 0 < counts["far"] < counts["all"] and 0 < counts["band"] < min(counts["near"], counts["far"])
    assert len(set(volumes.values())) == 4


def test_five_frames_with_max_weight_3_and_reset():
    vp = VC.box_volume((8, 8, 8), max_weight=3)
    dv, ov = make(vp)
    for f in range(5):
        img, intr = VC.box_frame(vp, 24, 40, seed=f)
        integrate_both(dv, ov, img, intr, np.eye(4), what=f"cap frame {f}")
    d, w = dv.read()
    assert w.max() == 3 and set(np.unique(w)) <= {0, 1, 2, 3}
    info = dv.info()
    assert info["integrations"] == 5 and info["dims"] == (8, 8, 8) and info["device_bytes"] >= 8 * 512
    assert info["voxel"] == F32(vp["voxel"]) and info["trunc"] == F32(vp["trunc"]) and info["origin"] == tuple(vp["origin"])
    dv.reset()
    d, w = dv.read()
    assert (d == F32(1)).all() and not w.any() and dv.info()["integrations"] == 0
    # a volume nobody integrated raycasts to zeros and extracts an empty cloud
    depth, normals, st = dv.raycast((17, 33), (40.0, 40.0, 16.0, 8.0), np.eye(4), params=ray_params(vp), return_normals=True, return_stats=True)
    assert not depth.any() and not normals.any() and st["n_hits"] == 0 and (st["n_launches"], st["n_host_syncs"]) == (1, 1)
    cloud, st = dv.extract(return_stats=True)
    assert len(cloud) == 0 and st["n_rows"] == 0 and (st["n_launches"], st["n_host_syncs"]) == (7, 2)


def test_the_sphere_at_64_cubed():
    """64^3 once: the four sphere views, the raycast at a size and intrinsics that are not the input's, and the extraction"""
    dv, ov = make(VC.SPHERE_VOLUME)
    intr = cases.intrinsics()
    for f, T in zip(VC.sphere_frames(), VC.SPHERE_VIEWS):
        integrate_both(dv, ov, f, intr, T, what="sphere")
    raycast_both(dv, ov, (60, 80), cases.intrinsics(60, 80, 70.0), VC.look(-0.2, 0.3), VC.SPHERE_RAYCAST, what="sphere raycast")
    xst = extract_both(dv, ov, what="sphere extract")
    assert xst["n_rows"] > 3000


def test_torch_tensors_on_a_side_stream():
    import torch
    vp = VC.box_volume((33, 9, 6))
    dv, ov = make(vp)
    side = torch.cuda.Stream()
    rp = ray_params(vp)
    with torch.cuda.stream(side):
        for f, dtype in enumerate((F32, np.uint16, F32)):
            img, intr = VC.box_frame(vp, 25, 41, seed=f, dtype=dtype)
            dev = torch.from_numpy(np.ascontiguousarray(img)).cuda()
            integrate_both(dv, ov, dev, intr, VC.box_pose(vp, "moved", seed=f), what=f"tensor frame {f}")
        wide = torch.zeros((25, 48), dtype=torch.float32, device="cuda")   # a tensor whose rows are 48 elements apart
        wide[:, 3:44] = torch.from_numpy(VC.box_frame(vp, 25, 41, seed=3)[0]).cuda()
        integrate_both(dv, ov, wide[:, 3:44], VC.box_frame(vp, 25, 41, seed=3)[1], np.eye(4), what="strided tensor")
        out = torch.empty((17, 33), dtype=torch.float32, device="cuda")
        raycast_both(dv, ov, (17, 33), (45.0, 44.0, 16.2, 8.0), VC.box_pose(vp, "moved", seed=2), rp, what="tensor raycast", out=out)
    side.synchronize()


@pytest.mark.parametrize("shape", [(17, 33), (16, 32)], ids=["17x33", "16x32"])
def test_raycast_device_writes_only_its_outputs(shape):
    """depth and normals inside canary arenas at 0 to 3 elements past an aligned address"""
    from test_gpu_device_outputs import Arena
    vp = VC.box_volume((33, 9, 6))
    dv, ov = make(vp)
    for f in range(2):
        img, intr = VC.box_frame(vp, 24, 40, seed=f)
        integrate_both(dv, ov, img, intr, np.eye(4))
    rp, rintr, pose = ray_params(vp), (45.0, 44.0, 16.2, 8.0), VC.box_pose(vp, "moved", seed=2)
    wd, wn, wst = O.raycast(ov, shape, rintr, pose, normals=True, **rp)
    assert wst["n_hits"] > 0
    n = shape[0] * shape[1]
    prm = _capi.DepthVolumeRaycastParams()
    lib().ppf_default_depth_volume_raycast_params(C.byref(prm))
    prm.z_near, prm.z_far = rp["z_near"], rp["z_far"]
    it, T = (C.c_double * 4)(*rintr), (C.c_double * 16)(*pose.reshape(-1))
    for pre in range(4):
        a, b = Arena(pre, n), Arena((pre + 1) % 4, n * 3)
        st = _capi.DepthVolumeRaycastStats()
        _capi.check(lib().ppf_depth_volume_raycast_device(dv._ptr, shape[0], shape[1], it, T, C.byref(prm), C.c_void_p(a.ptr), C.c_void_p(b.ptr),
                                                          None, C.byref(st)))
        a.check(wd, f"raycast depth +{pre}")
        b.check(wn, f"raycast normals +{(pre + 1) % 4}")
        assert (st.n_hits, st.n_interpolated) == (wst["n_hits"], wst["n_interpolated"])


@pytest.mark.parametrize("mode", [1, 2])
def test_the_helper_under_the_pool_guard(mode):
    from test_gpu_pool_guard import run_guarded
    run_guarded(mode, check_box, (33, 9, 6))
    run_guarded(mode, check_box, (7, 5, 3), (25, 41), np.uint16)


def test_twice_and_from_two_threads():
    first = check_box((33, 9, 6))
    assert check_box((33, 9, 6)) == first
    errors = []

    def work(dims):
        try:
            for _ in range(2):
                check_box(dims)
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(d,)) for d in ((33, 9, 6), (8, 8, 8))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_launches_and_syncs_do_not_depend_on_the_images():
    vp = VC.box_volume((8, 8, 8))
    dv = make(vp)[0]
    seen = set()
    for img in (np.zeros((24, 40), F32), VC.box_frame(vp, 24, 40, 0)[0], np.full((24, 40), np.nan, F32)):
        st = dv.integrate(img, VC.box_frame(vp, 24, 40, 0)[1], np.eye(4), return_stats=True)
        rst = dv.raycast((17, 33), (45.0, 44.0, 16.2, 8.0), np.eye(4), params=ray_params(vp), return_stats=True)[1]
        xst = dv.extract(return_stats=True)[1]
        seen.add((st["n_launches"], st["n_host_syncs"], rst["n_launches"], rst["n_host_syncs"], xst["n_launches"], xst["n_host_syncs"]))
    assert seen == {(1, 1, 1, 1, 7, 2)}


def test_device_entries_refuse_host_pointers_and_overlaps():
    import torch
    vp = VC.box_volume((8, 8, 8))
    dv, ov = make(vp)
    img, intr = VC.box_frame(vp, 24, 40, 0)
    integrate_both(dv, ov, img, intr, np.eye(4))
    before = dv.read()
    dp = _capi.DepthParams()
    lib().ppf_default_depth_params(C.byref(dp))
    it, T = (C.c_double * 4)(*intr), (C.c_double * 16)(*np.eye(4).reshape(-1))
    st = _capi.DepthVolumeIntegrateStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    s = lib().ppf_depth_volume_integrate_device(dv._ptr, img.ctypes.data, 24, 40, 0, it, C.byref(dp), T, None, C.byref(st))
    assert s == _capi.PPF_ERR_INVALID and "not device memory" in _capi.last_error() and bytes(st) == bytes(C.sizeof(st))
    dev = torch.from_numpy(img).cuda()
    # 160 MiB of rows from a tensor of 4 KB: past the end of whatever block the tensor was carved from
    s = lib().ppf_depth_volume_integrate_device(dv._ptr, C.c_void_p(dev.data_ptr()), 1 << 20, 40, 0, it, C.byref(dp), T, None, C.byref(st))
    assert s == _capi.PPF_ERR_INVALID and "runs past the end" in _capi.last_error()
    after = dv.read()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and dv.info()["integrations"] == 1
    # raycast: a host output, a short buffer, the normals over the depth
    prm = _capi.DepthVolumeRaycastParams()
    lib().ppf_default_depth_volume_raycast_params(C.byref(prm))
    rst = _capi.DepthVolumeRaycastStats()
    host = np.full((17, 33), 7.0, F32)
    ray = lambda d, n: lib().ppf_depth_volume_raycast_device(dv._ptr, 17, 33, it, T, C.byref(prm), d, n, None, C.byref(rst))
    assert ray(host.ctypes.data, None) == _capi.PPF_ERR_INVALID and "depth output" in _capi.last_error() and (host == 7.0).all()
    buf = torch.full((17 * 33 * 3 + 8,), 7.0, dtype=torch.float32, device="cuda")
    big = lib().ppf_depth_volume_raycast_device(dv._ptr, 4096, 4096, it, T, C.byref(prm), C.c_void_p(buf.data_ptr()), None, None, C.byref(rst))
    assert big == _capi.PPF_ERR_INVALID and "runs past the end" in _capi.last_error()     # a 64 MiB image into a 7 KB tensor
    assert ray(C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 16)) == _capi.PPF_ERR_INVALID and "overlaps" in _capi.last_error()
    assert ray(C.c_void_p(buf.data_ptr()), host.ctypes.data) == _capi.PPF_ERR_INVALID and "normals output" in _capi.last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 7.0).all() and bytes(rst) == bytes(C.sizeof(rst))


def test_depth_fusion_follows_the_oracle_chain():
    """four frames: the fused pose's bytes are the oracle chain's; then a frame it cannot follow leaves pose and volume alone"""
    frames, poses = cases.stream(4, 5, 20.0, 2.0)
    intr = cases.intrinsics()
    vp = VC.SCENE_VOLUME
    fus = DepthFusion(VC.SHAPE[0], VC.SHAPE[1], intr, make(vp)[0], raycast_params=VC.SCENE_RAYCAST)
    ora = O.Fusion(VC.SHAPE, intr, O.Volume(**vp), raycast_params=VC.SCENE_RAYCAST)
    for i, f in enumerate(frames):
        T, status = fus.push(f)
        Tw, sw = ora.push(f)
        assert status == sw and T.tobytes() == Tw.tobytes() and fus.pose.tobytes() == ora.pose.tobytes(), i
        if i:
            assert fus.model_depth.tobytes() == ora.model_depth.tobytes()
    same_voxels(fus.volume, ora.vol, "fused volume")
    err = MO.pose_error(fus.pose, poses[-1])
    assert err[0] <= 2 * 0.86 and err[1] <= 2 * 0.019      # tests/test_depth_volume_oracle.py measures the bound
    pose, integrations = fus.pose.copy(), fus.volume.info()["integrations"]
    T, status = fus.push(np.zeros(VC.SHAPE, F32))            # nothing to see: LOST
    assert status in (_capi.PPF_MOTION_LOST, _capi.PPF_MOTION_STEP) and T.tobytes() == np.eye(4).tobytes()
    assert fus.pose.tobytes() == pose.tobytes() and fus.volume.info()["integrations"] == integrations
    same_voxels(fus.volume, ora.vol, "after the lost frame")


@pytest.mark.parametrize("route", ["numpy", "tensor"])
def test_depth_fusion_on_uint16_frames(route):
    """uint16 frames are tracked as float32 metres and integrated as they came: three frames as numpy arrays and as GPU tensors
    against the oracle chain's bytes; float32 tensors take the same route as float32 arrays"""
    import torch
    frames, _ = cases.stream(3, 5, 20.0, 2.0)
    intr = cases.intrinsics()
    for dtype in (np.uint16, F32):
        if dtype == F32 and route == "numpy":
            continue   # test_depth_fusion_follows_the_oracle_chain
        imgs = [cases.to_u16(f, 0.0005) if dtype == np.uint16 else f for f in frames]
        fus = DepthFusion(VC.SHAPE[0], VC.SHAPE[1], intr, make(VC.SCENE_VOLUME)[0], raycast_params=VC.SCENE_RAYCAST, depth_scale=0.0005)
        ora = O.Fusion(VC.SHAPE, intr, O.Volume(**VC.SCENE_VOLUME), raycast_params=VC.SCENE_RAYCAST, depth_scale=0.0005)
        for i, f in enumerate(imgs):
            T, status = fus.push(torch.from_numpy(f).cuda() if route == "tensor" else f)
            Tw, sw = ora.push(f)
            assert status == sw and status in ((MO.NONE,) if i == 0 else (MO.CONVERGED, MO.MAX_ITERS)), (dtype, i, status, sw)
            assert T.tobytes() == Tw.tobytes() and fus.pose.tobytes() == ora.pose.tobytes(), (dtype, i)
        model = fus.model_depth.cpu().numpy() if route == "tensor" else fus.model_depth
        assert (route == "tensor") == type(fus.model_depth).__module__.startswith("torch")
        assert model.tobytes() == ora.model_depth.tobytes()
        same_voxels(fus.volume, ora.vol, f"fused {dtype.__name__} {route}")


def test_cpp_demo_matches_the_python_route(tmp_path):
    """examples/depth_volume_demo.cpp on three frames: its fused poses, the digest of its raycast image and its cloud's rows
    are the Python route's"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "yolo_ppf_pose_estimation_amd", "csrc")
    frames, _ = cases.stream(3, 5, 20.0, 2.0)
    intr = cases.intrinsics()
    vp, rp = VC.SCENE_VOLUME, VC.SCENE_RAYCAST
    exe = str(tmp_path / "depth_volume_demo")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "depth_volume_demo.cpp"), "-L", csrc, "-lppf_hip", f"-Wl,-rpath,{csrc}", "-o", exe], check=True)
    np.concatenate([f.reshape(-1) for f in frames]).astype("<f4").tofile(str(tmp_path / "frames.f32"))
    args = ([str(tmp_path / "frames.f32"), "3", str(VC.SHAPE[0]), str(VC.SHAPE[1])] + [repr(float(v)) for v in intr] + [str(d) for d in vp["dims"]] +
            [repr(float(F32(vp["voxel"])))] + [repr(float(v)) for v in vp["origin"]] + [repr(float(F32(vp["trunc"])))] +
            [repr(float(F32(rp["z_near"]))), repr(float(F32(rp["z_far"])))])
    r = subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    fmt = lambda T: " ".join("%.17g" % v for v in np.asarray(T).reshape(-1))
    vol = make(vp)[0]
    fus = DepthFusion(VC.SHAPE[0], VC.SHAPE[1], intr, vol, raycast_params=rp)
    want, ov = [], O.Volume(**vp)
    for k, f in enumerate(frames):
        T, status = fus.push(f)
        assert vol.info()["integrations"] == k + 1
        updated = O.integrate(ov, f, intr, fus.pose)     # the push does not return its count: the oracle's at the same pose
        want += [f"frame {k} status {status} updated {updated}", "  pose " + fmt(fus.pose)]
    same_voxels(vol, ov, "the demo's stream")
    image, st = vol.raycast(VC.SHAPE, intr, fus.pose, params=rp, return_stats=True)
    h = 14695981039346656037
    for b in image.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    cloud, xst = vol.extract(return_stats=True)
    want += [f"raycast hits {st['n_hits']} interpolated {st['n_interpolated']} digest {h:016x}",
             f"cloud rows {len(cloud)} of {xst['n_crossings']} crossings, 3 integrations"]
    assert len(lines) == len(want), r.stdout
    assert lines == want, r.stdout
    assert st["n_hits"] > 0 and len(cloud) > 0 and not np.array_equal(fus.pose, np.eye(4))


def test_fuse_volume_then_refine_frame():
    """the pose of frame 1 carried into frame 2 by the fused camera motion, then refined there (the bound of
    tests/test_gpu_depth_motion.py's TrackCamera test: 3 mm)"""
    import refine_oracle as R
    from test_gpu_depth_motion import tracking_frames
    d1, d2, model, T_obj, T_cam = tracking_frames()
    intr = cases.intrinsics()
    cp = CloudProcessor(None, d1, [], [], [], 0.05, 0.05)
    cp.LoadSingleModel(model, "ellipsoid")
    cp._model_clouds[0] = DeviceCloud.upload(model)
    cp.frame_intr, cp.frame_labels = intr, ["ellipsoid"]
    start = Pose3D()
    start.pose = T_obj.copy()
    cp.frame_poses = [[start]]
    vol = make(VC.SCENE_VOLUME)[0]
    T, status = cp.FuseVolume(d1, volume=vol, raycast_params=VC.SCENE_RAYCAST)
    assert status == _capi.PPF_MOTION_NONE and cp.frame_poses[0][0].pose.tobytes() == T_obj.tobytes()
    T, status = cp.FuseVolume(d2)
    ora = O.Fusion(VC.SHAPE, intr, O.Volume(**VC.SCENE_VOLUME), raycast_params=VC.SCENE_RAYCAST)
    ora.push(d1)
    Tw, sw = ora.push(d2)
    assert status == sw == MO.CONVERGED and T.tobytes() == Tw.tobytes() == cp.camera_motion.tobytes()
    assert cp.camera_pose.tobytes() == ora.pose.tobytes() and "fuse_volume" in cp.timings
    carried = cp.frame_poses[0][0]
    assert carried.pose.tobytes() == _mat44_mul(Tw, T_obj).tobytes()
    # once the fusion exists its keywords and a frame of another shape are refused; nothing moves
    for bad in (dict(depth=d2, raycast_params=VC.SCENE_RAYCAST), dict(depth=d2[:, :-1])):
        with pytest.raises(_capi.PPFError) as e:
            cp.FuseVolume(**bad)
        assert e.value.status == _capi.PPF_ERR_INVALID and "FuseVolume" in str(e.value)
    assert vol.info()["integrations"] == 2 and cp.camera_pose.tobytes() == ora.pose.tobytes()
    cp.RefineFrame(depth=d2)
    d_refined = R.mean_row_error(model, cp.frame_poses[0][0].pose, T_cam @ T_obj)
    print(f"ellipsoid: {d_refined * 1e3:.2f} mm after FuseVolume and RefineFrame")
    assert cp.refine_info[0, 0]["status"] in (R.CONVERGED, R.MAX_ITERS) and d_refined <= 0.003


def test_scan_train_match():
    """a smoke check of the loop, no accuracy claim: a sphere and an ellipsoid scanned from four sides, the extracted cloud
    trained on, and one view of them matched"""
    dv = make(VC.SPHERE_VOLUME)[0]
    intr = cases.intrinsics()
    for T in VC.SPHERE_VIEWS:
        dv.integrate(VC.render_scan(T), intr, T)
    model = dv.extract().rows()
    assert len(model) > 2000 and np.isfinite(model).all()
    det = PPF3DDetector(0.05, 0.05)
    det.trainModel(model)
    scene = DeviceCloud.from_depth(VC.render_scan(VC.SPHERE_VIEWS[1]), intr, normals=dict(drop=True)).rows()
    poses = det.match(scene, 1.0 / 10.0, 0.05)
    assert len(poses) >= 1


def test_depth_odometry_is_untouched_by_the_volume():
    """the frame-to-frame chain beside a fusion on the same frames: DepthOdometry's poses are what they were"""
    frames, _ = cases.stream(3, 5, 20.0, 2.0)
    intr = cases.intrinsics()
    odo = DepthOdometry(VC.SHAPE[0], VC.SHAPE[1], intr)
    fus = DepthFusion(VC.SHAPE[0], VC.SHAPE[1], intr, make(VC.SCENE_VOLUME)[0], raycast_params=VC.SCENE_RAYCAST)
    chain = np.eye(4)
    for i, f in enumerate(frames):
        odo.push(f)
        fus.push(f)
        if i:
            chain = O.mat44_mul(MO.motion(frames[i - 1], f, intr)[0], chain)
    assert odo.pose.tobytes() == chain.tobytes()
