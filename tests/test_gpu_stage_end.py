"""The end of a stage call that fails after its first launch (FrameRun::finish and stage_entry).

For each stage that can fail that late: a good call, whose output bytes are kept; the failing call, whose status, text, cleared
outputs and stats are what the entry documents; the same good call again at once, whose bytes equal the first call's -- the
scratch and the output block the failed call gave back hold nothing the next call can see; and the pool check, which reports
no damaged zone.  All of it plain and under the block cache's guard with the fill words 0 and 1 (test_gpu_pool_guard.py).

What this cannot show is the wait on failure itself: a missing wait is a race, and nothing here is run to provoke one.  That
part is read: it is stage_finish, in ppf_stage_host.h."""
import ctypes as C
import re

import numpy as np
import pytest

import mesh_oracle as MO
import region_cases as RC
import test_gpu_clusters as TC
import test_gpu_pool_guard as G
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import lib
from yolo_ppf_pose_estimation_amd.cloud_processor import DepthVolume, DeviceCloud, cluster_clouds, region_clouds

pytestmark = pytest.mark.gpu

POISON = 0x5A


def poisoned(record):
    C.memset(C.byref(record), POISON, C.sizeof(record))
    return record


def is_zero(record):
    return bytes(record) == bytes(C.sizeof(record))


def cloud_bytes(cloud):
    rows, curv = cloud.download()
    return rows.tobytes() + curv.tobytes()


# ---- ppf_prep_voxel_grid: the index overflow, found by the read-back after the sort's launches ------------------------------
VOXEL_XYZ = np.random.default_rng(41).uniform(-0.2, 0.2, (2000, 3)).astype(np.float32)


def voxel_good():
    return cloud_bytes(DeviceCloud.upload(VOXEL_XYZ).voxel_grid(0.01))


def voxel_bad():
    big = DeviceCloud.upload(VOXEL_XYZ * 1000)
    out = C.c_void_p(0x5A5A)
    assert lib().ppf_prep_voxel_grid(big._ptr, 1e-4, C.byref(out)) == _capi.PPF_ERR_INVALID
    assert _capi.last_error() == "ppf_prep_voxel_grid: leaf size is too small for the cloud (index overflow)"
    assert out.value is None


# ---- ppf_prep_clusters and ppf_prep_regions: a cloud that spans more cells than a grid axis has, found after the wait --------
NEAR = RC.rows6(TC.blobs([500, 500], seed=42))                 # two blobs 0.2 m apart
FAR = RC.rows6(TC.blobs([500, 500], seed=42, pitch=100.0))     # 100 m apart: thousands of cells at tolerance 0.02, 1,024 allowed
TOL = float(np.float32(0.02))                                  # the params hold a float
LABEL_STAGES = {"clusters": (cluster_clouds, "ppf_prep_clusters", _capi.ClusterParams, "ppf_default_cluster_params", "max_clusters", 3),
                "regions": (region_clouds, "ppf_prep_regions", _capi.RegionParams, "ppf_default_region_params", "max_regions", 4)}


def labels_good(which):
    call, _, _, _, max_field, n_counts = LABEL_STAGES[which]
    dev = DeviceCloud.upload(NEAR, curvature=np.zeros(len(NEAR), np.float32))
    found, info, counts, labels, st = call([dev], {"tolerance": 0.02, max_field: 4}, return_info=True, return_labels=True)
    assert counts.shape == (1, n_counts) and list(counts[0, :3]) == [2, 2, 2] and st["n_host_syncs"] == 1 and st["n_launches"] > 100
    return info.tobytes() + counts.tobytes() + labels[0].tobytes() + b"".join(cloud_bytes(c) for c in found[0])


def labels_bad(which):
    _, entry, params, defaults, max_field, n_counts = LABEL_STAGES[which]
    dev = DeviceCloud.upload(FAR, curvature=np.zeros(len(FAR), np.float32))
    prm = params()
    getattr(lib(), defaults)(C.byref(prm))
    prm.tolerance = 0.02
    setattr(prm, max_field, 4)
    ins, outs = (C.c_void_p * 1)(dev._ptr), (C.c_void_p * 4)(*[0x5A5A] * 4)
    info, counts = poisoned((_capi.ClusterInfo * 4)()), poisoned((C.c_int32 * n_counts)())
    labels = np.full(len(FAR), 77, np.int32)
    lab, st = (C.c_void_p * 1)(labels.ctypes.data), poisoned(_capi.ClusterStats())
    s = getattr(lib(), entry)(ins, 1, C.byref(prm), None, 0, 0, outs, info, counts, lab, C.byref(st))
    assert s == _capi.PPF_ERR_INVALID
    m = re.fullmatch(entry + r": in\[0\] spans (\S+) m, (\d+) cells of its grid on an axis \(at most 1024\); "
                     r"the smallest tolerance that fits is (\S+)", _capi.last_error())
    extent = float((FAR[:, :3].max(axis=0).astype(np.float64) - FAR[:, :3].min(axis=0).astype(np.float64)).max())
    assert m and m.group(1) == "%g" % extent and int(m.group(2)) == int(extent / (TOL * 0.5773)) + 1, _capi.last_error()
    assert TOL * int(m.group(2)) / 1024 * 0.99 < float(m.group(3)) < TOL * int(m.group(2)) / 1024 * 1.01
    assert list(outs) == [None] * 4 and is_zero(info) and is_zero(counts) and is_zero(st)
    assert (labels == 77).all()      # the labels of a failed call are not written


# ---- ppf_cloud_from_mesh: the device-side capacity error, after the sizing wait -------------------------------------------
def strip(n_triangles, step=0.004):
    """a flat zig-zag strip: n + 2 vertices, triangle k = (k, k + 1, k + 2)"""
    i = np.arange(n_triangles + 2)
    V = np.stack([(i // 2) * step, (i % 2) * step, np.zeros(len(i))], axis=1).astype(np.float32)
    T = np.stack([i[:-2], i[1:-1], i[2:]], axis=1).astype(np.int32)
    return V, T


MESH_V, MESH_T = strip(_capi.PPF_MESH_HOST_COUNT + 1)
MESH_SPACING = 0.002


def mesh_yield():
    """checked on the CPU: what the oracle samples from the strip, which the failing call's max_rows is one below"""
    n = int(MO.mesh_sample(MESH_V, MESH_T, MESH_SPACING, visibility=0, orient=0)["stats"]["n_sampled"])
    assert len(MESH_T) == _capi.PPF_MESH_HOST_COUNT + 1 and 1 < n < (1 << 24)
    return n


def mesh_good():
    cloud, st = DeviceCloud.from_mesh(MESH_V, MESH_T, MESH_SPACING, map_size=64, max_rows=mesh_yield(), return_stats=True)
    assert (st["n_launches"], st["n_host_syncs"], st["n_sampled"]) == (17, 2, mesh_yield())
    return cloud_bytes(cloud)


def mesh_bad():
    prm, st, out = _capi.MeshSampleParams(), poisoned(_capi.MeshSampleStats()), C.c_void_p(0x5A5A)
    lib().ppf_default_mesh_sample_params(C.byref(prm))
    prm.spacing, prm.map_size, prm.max_rows = MESH_SPACING, 64, mesh_yield() - 1
    s = lib().ppf_cloud_from_mesh(MESH_V.ctypes.data, len(MESH_V), 3, -1, MESH_T.ctypes.data, len(MESH_T), C.byref(prm), C.byref(out), C.byref(st))
    assert s == _capi.PPF_ERR_CAPACITY
    assert _capi.last_error() == "ppf_cloud_from_mesh: the mesh gives more than max_rows = %d rows at spacing 0.002" % (mesh_yield() - 1)
    assert out.value is None and is_zero(st)


# ---- ppf_depth_volume_mesh: a shell without device memory, through stage_entry ----------------------------------------------
VOLUME_DIMS = (16, 16, 16)


def sphere_volume():
    vol = DepthVolume(VOLUME_DIMS, 0.01, (0.0, 0.0, 0.5), trunc=0.04, max_weight=8)
    z, y, x = np.meshgrid(*[np.arange(16, dtype=np.float64)] * 3, indexing="ij")
    d = (np.sqrt((x - 7.3) ** 2 + (y - 7.6) ** 2 + (z - 7.9) ** 2) * 0.01 - 0.05) / 0.04
    vol.write(np.clip(d, -1.0, 1.0).astype(np.float32), np.full(d.shape, 3, np.int32))
    return vol


def volume_good():
    m, st = sphere_volume().mesh(return_stats=True)
    assert st["n_triangles"] > 100 and st["n_host_syncs"] == 2
    return m.vertices().tobytes() + m.triangles().tobytes()


def volume_bad():
    vp = _capi.DepthVolumeParams()
    lib().ppf_default_depth_volume_params(C.byref(vp))
    vp.dims[:] = VOLUME_DIMS
    shell = C.c_void_p()
    _capi.check(lib().ppf_debug_depth_volume_shell(C.byref(vp), C.byref(shell)))
    try:
        mp, st, out = _capi.DepthVolumeMeshParams(), poisoned(_capi.DepthVolumeMeshStats()), C.c_void_p(0x5A5A)
        lib().ppf_default_depth_volume_mesh_params(C.byref(mp))
        assert lib().ppf_depth_volume_mesh(shell, C.byref(mp), C.byref(out), C.byref(st)) == _capi.PPF_ERR_INVALID
        assert _capi.last_error() == "ppf_depth_volume_mesh: the volume is a shell without device memory"
        assert out.value is None and is_zero(st)
    finally:
        assert lib().ppf_depth_volume_release(shell) == _capi.PPF_OK


CASES = {"voxel_grid": (voxel_good, voxel_bad),
         "clusters": (lambda: labels_good("clusters"), lambda: labels_bad("clusters")),
         "regions": (lambda: labels_good("regions"), lambda: labels_bad("regions")),
         "cloud_from_mesh": (mesh_good, mesh_bad),
         "volume_mesh": (volume_good, volume_bad)}


def good_bad_good(name):
    good, bad = CASES[name]
    first = good()
    bad()
    assert good() == first, name


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["plain", "guard 1", "guard 2"])
@pytest.mark.parametrize("name", list(CASES))
def test_a_failed_call_leaves_nothing_behind(name, mode):
    if mode:
        G.run_guarded(mode, good_bad_good, name)
    else:
        good_bad_good(name)
        assert G.pool_check()[1] == []
