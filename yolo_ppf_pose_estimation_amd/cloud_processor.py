"""Host-side mirror of the reference's ``ppf::CloudProcessor`` (/root/reference/include/CloudProcessing.h) over the
C-ABI: the PCL stages that produce the matcher's N x 6 input (SceneCropping :263, Subsampling :361, OutlierProcessing
:341, NormalEstimation :381, EdgeExtraction :406, PointCloudXYZNormalToMat :163) followed by the PPF calls
(LoadSingleModel :209, TrainDetector :222, Matching :428, Matching_S2B :481, with the ICP step).  Clouds stay on the
device between stages (``DeviceCloud`` wraps a ``ppf_cloud*``).  Method names, argument order and defaults are the
reference's; the YOLO detector that supplies ``boxes`` is out of scope."""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _capi
from ._capi import (ClusterInfo, ClusterParams, ClusterStats, RegionParams, FrameDetection, FrameParams, FrameStats, IcpParams, MatchFrameStats, PlaneInfo, PlaneParams, PlaneStats, Pose,
                    PoseScore, PPFError, RefineInfo,
                    RefineParams, RefineStats, RenderParams, RenderStats, SelectInfo, SelectParams, SelectStats, VerifyParams, VerifyStats,
                    check, lib)
from .detector import ICP, PPF3DDetector, Pose3D


class DeviceCloud:
    """A device-resident cloud (rows ``x y z nx ny nz`` + curvature)."""

    def __init__(self, ptr):
        self._ptr = ptr

    @classmethod
    def upload(cls, rows: np.ndarray, normal_offset: int = 3, curvature=None) -> "DeviceCloud":
        """rows: N x 3 (xyz) or N x 6 (xyz + normal); curvature: None (zero) or N float32 (ppf_cloud_set_curvature)"""
        a = np.ascontiguousarray(rows, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise PPFError(_capi.PPF_ERR_INVALID, "cloud must be N x 3 (xyz) or N x 6 (xyz + normal) float32")
        cols = 6 if a.shape[1] >= 6 else 3
        out = C.c_void_p()
        check(lib().ppf_cloud_upload(a.ctypes.data, a.shape[0], a.shape[1], normal_offset, cols, C.byref(out)))
        cloud = cls(out)
        if curvature is not None:
            c = np.ascontiguousarray(curvature, dtype=np.float32).reshape(-1)
            check(lib().ppf_cloud_set_curvature(cloud._ptr, c.ctypes.data, c.shape[0]))
        return cloud

    @classmethod
    def from_depth(cls, depth, intr, *, depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0,
                   fp64: bool = False, normals: Optional[dict] = None, filter: Optional[dict] = None, edges: Optional[dict] = None):
        """The organised scene cloud of a depth image, back-projected on the device (ppf_cloud_from_depth): rows
        ``x y z 0 0 0`` of every pixel with a finite z > 0 inside [z_min, z_max] (z_max 0: no upper bound), in row-major
        pixel order.  depth: a 2-D numpy float32 (metres) or uint16 (units of depth_scale metres) array, rows read at its
        stride; or a float32 / uint16 torch tensor on the GPU, read in place on ``torch.cuda.current_stream()``.
        intr: (fx, fy, ppx, ppy) or the 3x3 camera matrix.  fp64=True: the fp64 formula instead of
        Camera::back_projection's rounding.  normals: None, or a dict with any of radius,
        max_depth_change, min_neighbours, drop (ppf_cloud_from_depth_normals): the same rows with the normal
        and curvature of a plane fit over each pixel's (2 radius + 1)^2 image window; a pixel with fewer than
        min_neighbours neighbours gets NaNs, or with drop=True no row.  filter: None, or a dict of ppf_depth_filter_params
        fields ({}: the defaults): the image goes through ``filter_depth`` first -- on the device and the
        current stream for a GPU tensor -- and the cloud is built from the filtered float32 image with the same z_min and
        z_max.  edges: None, or a dict of ppf_depth_edge_params fields ({}: the defaults): the result is then
        ``(cloud, edge_cloud)``, the second being ``depth_edges``' cloud of the same (filtered) image, with
        the cloud as its normals when ``normals`` is given without drop."""
        if filter is not None:
            depth = filter_depth(depth, depth_scale=depth_scale, z_min=z_min, z_max=z_max, params=filter)
        K = np.asarray(intr, dtype=np.float64)
        it = (C.c_double * 4)(*([K[0, 0], K[1, 1], K[0, 2], K[1, 2]] if K.shape == (3, 3) else [float(v) for v in K.reshape(-1)[:4]]))
        prm = _depth_params(depth_scale, z_min, z_max, _capi.PPF_DEPTH_FP64 if fp64 else 0)
        nprm = None
        if normals is not None:
            unknown = set(normals) - {"radius", "max_depth_change", "min_neighbours", "drop"}
            if unknown:
                raise PPFError(_capi.PPF_ERR_INVALID, f"normals: unknown keys {sorted(unknown)}")
            nprm = _capi.DepthNormalParams()
            lib().ppf_default_depth_normal_params(C.byref(nprm))
            nprm.radius = int(normals.get("radius", nprm.radius))
            nprm.max_depth_change = float(normals.get("max_depth_change", nprm.max_depth_change))
            nprm.min_neighbours = int(normals.get("min_neighbours", nprm.min_neighbours))
            nprm.flags = _capi.PPF_DEPTH_NORMALS_DROP if normals.get("drop", False) else 0
        inp = _DepthInput(depth, "depth must be a 2-D float32 or uint16 {kind}")
        prm.format = inp.format
        out = C.c_void_p()
        name = "ppf_cloud_from_depth" + ("_normals" if nprm is not None else "") + ("_device" if inp.is_device else "")
        with inp.device():
            tail = (() if nprm is None else (C.byref(nprm),)) + ((inp.stream(),) if inp.is_device else ())
            check(getattr(lib(), name)(inp.ptr, inp.rows, inp.cols, inp.pitch, it, C.byref(prm), *tail, C.byref(out)))
        made = cls(out)
        if edges is None:
            return made
        nrm = made if nprm is not None and not nprm.flags & _capi.PPF_DEPTH_NORMALS_DROP else None
        _, edge = depth_edges(depth, intr, depth_scale=depth_scale, z_min=z_min, z_max=z_max, fp64=fp64, normals=nrm, params=edges, cloud=True)
        return made, edge

    @classmethod
    def from_mesh(cls, vertices, triangles, spacing: float, *, seed: int = 0, normals: str = "face", visibility: bool = True,
                  orient: bool = True, map_size: int = 0, min_views: int = 0, depth_tol: float = 0.0, max_rows: int = 0,
                  return_stats: bool = False, normal_offset: Optional[int] = None):
        """A model cloud sampled from a triangle mesh (ppf_cloud_from_mesh): on average one row per
        spacing^2 of surface, rows ``x y z nx ny nz``.  vertices: (N, 3) float32, or (N, >= 6) with the vertex normals in
        the last three columns (or at column normal_offset); triangles: (M, 3) int32.  normals: "face", or "vertex" to interpolate the vertex normals.
        visibility: drop the rows none of 26 orthographic views of map_size^2 pixels (0: 256) can see -- inner walls, double
        shells -- keeping those seen by at least min_views (0: 1) within depth_tol metres (0: two map pixels); orient: turn
        a normal that more views see from behind, which mends inconsistent winding.  More than max_rows (0: 2^24) sampled
        rows is PPF_ERR_CAPACITY.  The rows depend on the arguments alone: a seed names a cloud."""
        V = np.ascontiguousarray(vertices, dtype=np.float32)
        T = np.ascontiguousarray(triangles, dtype=np.int32)
        if V.ndim != 2 or T.ndim != 2 or T.shape[1] != 3:
            raise PPFError(_capi.PPF_ERR_INVALID, "from_mesh: vertices must be (N, 3 | >= 6) float32 and triangles (M, 3) int32")
        if normals not in ("face", "vertex"):
            raise PPFError(_capi.PPF_ERR_INVALID, f"from_mesh: normals must be 'face' or 'vertex', not {normals!r}")
        prm = _capi.MeshSampleParams()
        lib().ppf_default_mesh_sample_params(C.byref(prm))
        prm.spacing, prm.seed = float(spacing), int(seed) & 0xFFFFFFFF
        prm.normals = _capi.PPF_MESH_NORMALS_VERTEX if normals == "vertex" else _capi.PPF_MESH_NORMALS_FACE
        prm.visibility, prm.orient = int(bool(visibility)), int(bool(orient))
        prm.map_size, prm.min_views, prm.depth_tol, prm.max_rows = int(map_size), int(min_views), float(depth_tol), int(max_rows)
        noff = int(normal_offset) if normal_offset is not None else (V.shape[1] - 3 if V.shape[1] >= 6 else -1)
        out, st = C.c_void_p(), _capi.MeshSampleStats()
        check(lib().ppf_cloud_from_mesh(V.ctypes.data, V.shape[0], V.shape[1], noff,
                                        T.ctypes.data, T.shape[0], C.byref(prm), C.byref(out), C.byref(st)))
        cloud = cls(out)
        return (cloud, _capi.stats_dict(st)) if return_stats else cloud

    def __del__(self):
        try:
            if self._ptr:
                lib().ppf_cloud_release(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def __len__(self) -> int:
        n = C.c_int(0)
        check(lib().ppf_cloud_size(self._ptr, C.byref(n)))
        return n.value

    size = __len__

    def download(self):
        """(rows (n, 6) float32, curvature (n,) float32)"""
        n = len(self)
        rows = np.zeros((n, 6), dtype=np.float32)
        curv = np.zeros(n, dtype=np.float32)
        check(lib().ppf_cloud_download(self._ptr, rows.ctypes.data, curv.ctypes.data, n))
        return rows, curv

    def rows(self) -> np.ndarray:
        return self.download()[0]

    def xyz(self) -> np.ndarray:
        return self.download()[0][:, :3].copy()

    def device_rows(self):
        """(device pointer, n): packed n x 6 rows for ppf_match_device / ppf_icp_refine_device"""
        p, n = C.c_void_p(), C.c_int(0)
        check(lib().ppf_cloud_device_rows(self._ptr, C.byref(p), C.byref(n)))
        return p.value, n.value

    def _stage(self, fn, *args) -> "DeviceCloud":
        out = C.c_void_p()
        check(fn(self._ptr, *args, C.byref(out)))
        return DeviceCloud(out)

    # the stages, one call each
    def crop(self, box, depth: np.ndarray, intr) -> "DeviceCloud":
        d = np.ascontiguousarray(depth, dtype=np.float32)
        bx = (C.c_int * 4)(*[int(v) for v in box])
        it = (C.c_double * 4)(*[float(v) for v in intr])
        return self._stage(lib().ppf_prep_crop, bx, d.ctypes.data, d.shape[0], d.shape[1], it)

    def voxel_grid(self, leaf: float) -> "DeviceCloud":
        return self._stage(lib().ppf_prep_voxel_grid, float(leaf))

    def outlier_removal(self, mean_k: int = 50, stddev_mul: float = 1.5) -> "DeviceCloud":
        return self._stage(lib().ppf_prep_outlier_removal, int(mean_k), float(stddev_mul))

    def normals(self, k: int = 30) -> "DeviceCloud":
        return self._stage(lib().ppf_prep_normals, int(k))

    def edges(self, curvature_threshold: float) -> "DeviceCloud":
        return self._stage(lib().ppf_prep_edges, C.c_float(curvature_threshold))

    def to_mat(self) -> "DeviceCloud":
        return self._stage(lib().ppf_prep_to_mat)

    def prep_frame(self, boxes, depth: np.ndarray, intr, params=None, *, return_info: bool = False):
        """every stage crop -> voxel grid -> outlier removal -> normals -> edges -> to-Mat for all boxes of the frame in one
        call (ppf_prep_frame): a list of (object, edge) DeviceCloud pairs, one per box, bit-identical to the per-box chain.
        params: a FrameParams, a dict of its fields (the rest default) or None (the defaults).  return_info=True also
        returns the rows per box after crop / voxel grid / outlier removal / edges ((K, 4) int32) and the call's stats."""
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
        nb = b.shape[0]
        prm = params
        if not isinstance(prm, FrameParams):
            prm = FrameParams()
            lib().ppf_default_frame_params(C.byref(prm))
            for key, v in (params or {}).items():
                setattr(prm, key, v)
        d = np.ascontiguousarray(depth, dtype=np.float32)
        it = (C.c_double * 4)(*[float(v) for v in intr])
        objs, edges = (C.c_void_p * max(nb, 1))(), (C.c_void_p * max(nb, 1))()
        rows = np.zeros((nb, 4), dtype=np.int32)
        st = FrameStats()
        check(lib().ppf_prep_frame(self._ptr, b.ctypes.data_as(C.POINTER(C.c_int)), nb, d.ctypes.data, d.shape[0], d.shape[1], it,
                                   C.byref(prm), objs, edges, rows.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st)))
        pairs = [(DeviceCloud(C.c_void_p(objs[i])), DeviceCloud(C.c_void_p(edges[i]))) for i in range(nb)]
        if return_info:
            return pairs, rows, _capi.stats_dict(st)
        return pairs

    def remove_planes(self, params=None, return_info: bool = False, return_labels: bool = False):
        """this cloud without its support planes (ppf_prep_planes with one cloud; see the module-level ``remove_planes``)"""
        res = remove_planes([self], params, return_info=return_info, return_labels=return_labels)
        if not (return_info or return_labels):
            return res[0]
        out = [part[0] for part in res[:1 + int(return_info) + int(return_labels)]]   # this cloud's kept rows, info rows, labels
        return tuple(out + [res[-1]] if return_info else out)                        # the stats last

    def apply_planes(self, info, params=None) -> "DeviceCloud":
        """the rows of this cloud (a detection's edge cloud) that the planes of ``info`` -- the info rows ``remove_planes``
        returned for one cloud -- do not remove (ppf_prep_planes_apply): same predicate, same ``params``"""
        prm = _params(PlaneParams, "ppf_default_plane_params", params, "plane")
        rec = np.ascontiguousarray(np.asarray(info, dtype=PLANE_INFO).reshape(-1))
        return self._stage(lib().ppf_prep_planes_apply, rec.ctypes.data_as(C.POINTER(PlaneInfo)), int(rec.shape[0]), C.byref(prm))

    def _labelled(self, fn, params, intr, image_size, return_info, return_labels):
        """``fn`` (cluster_clouds or region_clouds) on this cloud alone: its parts of the results, the stats last"""
        res = fn([self], params, intr, image_size, return_info=return_info, return_labels=return_labels)
        if not (return_info or return_labels):
            return res[0]
        n = 1 + 2 * int(return_info) + int(return_labels)   # this cloud's components, info rows, counts, labels
        out = [part[0] for part in res[:n]]
        return tuple(out + [res[-1]] if return_info else out)

    def clusters(self, params=None, intr=None, image_size=None, return_info: bool = False, return_labels: bool = False):
        """this cloud's object clusters (ppf_prep_clusters with one cloud; see the module-level ``cluster_clouds``)"""
        return self._labelled(cluster_clouds, params, intr, image_size, return_info, return_labels)

    def regions(self, params=None, intr=None, image_size=None, return_info: bool = False, return_labels: bool = False):
        """this cloud's smooth surface regions (ppf_prep_regions with one cloud; see the module-level ``region_clouds``)"""
        return self._labelled(region_clouds, params, intr, image_size, return_info, return_labels)

    def knn(self, k: int):
        n = len(self)
        idx = np.zeros((n, k), dtype=np.int32)
        d2 = np.zeros((n, k), dtype=np.float32)
        check(lib().ppf_prep_knn(self._ptr, int(k), idx.ctypes.data, d2.ctypes.data))
        return idx, d2


# ppf_plane_info as a numpy record
PLANE_INFO = np.dtype([("n", "<f8", 3), ("d", "<f8"), ("status", "<i4"), ("hypothesis", "<i4"), ("n_rows", "<i4"), ("n_hyp_inliers", "<i4"),
                       ("n_inliers", "<i4"), ("n_behind", "<i4"), ("refit", "<i4"), ("reserved", "<i4")])


def remove_planes(clouds, params=None, return_info: bool = False, return_labels: bool = False):
    """The support planes (the table, a wall) of every cloud found and removed in one segmented call (ppf_prep_planes):
    up to ``max_planes`` rounds of a seeded hypothesis search per cloud, each cloud's result byte-identical to a call with
    it alone.  params: a PlaneParams, a dict of its fields (the rest default) or None.  Returns the list of kept clouds; with
    return_info also the info rows ((n_clouds, max_planes) records of ``PLANE_INFO``) and, last, the call's stats; with
    return_labels the per-row labels (uint8: 0 kept, 1 + p inlier of plane p, 0x80 | (1 + p) behind plane p) per cloud."""
    prm = _params(PlaneParams, "ppf_default_plane_params", params, "plane")
    K = len(clouds)
    ins, outs = (C.c_void_p * max(K, 1))(*[c._ptr for c in clouds]), (C.c_void_p * max(K, 1))()
    info = np.zeros((K, max(1, min(int(prm.max_planes), _capi.PPF_PLANE_MAX_PLANES))), dtype=PLANE_INFO)
    labels = [np.zeros(len(c), dtype=np.uint8) for c in clouds] if return_labels else None
    lab = (C.c_void_p * max(K, 1))(*[a.ctypes.data for a in labels]) if return_labels else None
    st = PlaneStats()
    check(lib().ppf_prep_planes(ins, K, C.byref(prm), outs, info.ctypes.data_as(C.POINTER(PlaneInfo)), lab, C.byref(st)))
    kept = [DeviceCloud(C.c_void_p(outs[i])) for i in range(K)]
    if not (return_info or return_labels):
        return kept
    res = [kept]
    if return_info:
        res.append(info)
    if return_labels:
        res.append(labels)
    if return_info:
        res.append(_capi.stats_dict(st))
    return tuple(res)


# ppf_cluster_info as a numpy record
CLUSTER_INFO = np.dtype([("n_rows", "<i4"), ("first_row", "<i4"), ("lo", "<f4", 3), ("hi", "<f4", 3), ("box_xywh", "<i4", 4),
                         ("reserved", "<i4", 4)])


def cluster_clouds(clouds, params=None, intr=None, image_size=None, return_info: bool = False, return_labels: bool = False):
    """Euclidean cluster extraction of every cloud in one segmented call (ppf_prep_clusters): the connected components of
    "two rows are no farther apart than ``tolerance``" (fp64, ``<=``), those of ``min_size .. max_size`` rows ranked by size
    (then by their first row), the first ``max_clusters`` of them returned, each cloud's result byte-identical to a call
    with it alone.  params: a ClusterParams, a dict of its fields (the rest default) or None.  intr: (fx, fy, ppx, ppy) or
    the 3x3 matrix, with image_size = (rows, cols), gives every cluster its image box; without, the boxes are zero.
    Returns one list of cluster clouds per cloud; with return_info also the info rows ((n_clouds, max_clusters) records of
    ``CLUSTER_INFO``, zero past a cloud's count), the counts ((n_clouds, 3): clusters, valid components, all components) and,
    last, the call's stats; with return_labels the per-row labels (int32: the cluster's rank, or -1) per cloud."""
    return _label_clouds("cluster_clouds", lib().ppf_prep_clusters, _params(ClusterParams, "ppf_default_cluster_params", params, "cluster"),
                         "max_clusters", 3, clouds, intr, image_size, return_info, return_labels)


def region_clouds(clouds, params=None, intr=None, image_size=None, return_info: bool = False, return_labels: bool = False):
    """The smooth surface regions of every cloud in one segmented call (ppf_prep_regions): region growing on the normals the
    clouds carry, as a closed specification.  Rows of finite x, y, z and normal take part; those of curvature <=
    ``curvature_threshold`` are smooth, the others border rows.  Two smooth rows are linked iff they are no farther apart than
    ``tolerance`` and the dot product of their normals is >= ``normal_cos`` (both fp64; ``flags = PPF_REGION_UNORIENTED``: its
    absolute value); a region is a connected component of the links plus the border rows whose nearest linkable smooth row
    is in it.  Validity, ranking and the return values are ``cluster_clouds``', with ``max_regions`` for ``max_clusters``:
    one list of region clouds per cloud; with return_info also the info rows (``CLUSTER_INFO``; ``first_row`` is the region's
    smallest smooth row), the counts ((n_clouds, 4): regions, valid components, all components, border rows attached) and,
    last, the call's stats; with return_labels the per-row labels (int32: the region's rank, or -1) per cloud."""
    return _label_clouds("region_clouds", lib().ppf_prep_regions, _params(RegionParams, "ppf_default_region_params", params, "region"),
                         "max_regions", 4, clouds, intr, image_size, return_info, return_labels)


def _label_clouds(who, entry, prm, max_field, n_counts, clouds, intr, image_size, return_info, return_labels):
    """what ``cluster_clouds`` and ``region_clouds`` share: one call of ``entry`` (ppf_prep_clusters' signature) with the params
    record ``prm``, whose ``max_field`` bounds a cloud's components; ``n_counts`` words of counts per cloud"""
    K = len(clouds)
    mc = max(1, min(int(getattr(prm, max_field)), _capi.PPF_CLUSTER_MAX_CLUSTERS))
    ins, outs = (C.c_void_p * max(K, 1))(*[c._ptr for c in clouds]), (C.c_void_p * max(K * mc, 1))()
    info = np.zeros((K, mc), dtype=CLUSTER_INFO)
    counts = np.zeros((K, n_counts), dtype=np.int32)
    labels = [np.full(len(c), -1, dtype=np.int32) for c in clouds] if return_labels else None
    lab = (C.c_void_p * max(K, 1))(*[a.ctypes.data for a in labels]) if return_labels else None
    it, rows, cols = None, 0, 0
    if intr is not None:
        if image_size is None:
            raise PPFError(_capi.PPF_ERR_INVALID, f"{who}: intr needs image_size = (rows, cols)")
        it, (rows, cols) = (C.c_double * 4)(*_intr4(intr)), image_size
    st = ClusterStats()
    check(entry(ins, K, C.byref(prm), it, int(rows), int(cols), outs, info.ctypes.data_as(C.POINTER(ClusterInfo)),
                counts.ctypes.data_as(C.POINTER(C.c_int32)), lab, C.byref(st)))
    found = [[DeviceCloud(C.c_void_p(outs[i * mc + r])) for r in range(int(counts[i, 0]))] for i in range(K)]
    if not (return_info or return_labels):
        return found
    res = [found]
    if return_info:
        res += [info, counts]
    if return_labels:
        res.append(labels)
    if return_info:
        res.append(_capi.stats_dict(st))
    return tuple(res)


def _intr4(intr):
    K = np.asarray(intr, dtype=np.float64)
    return [K[0, 0], K[1, 1], K[0, 2], K[1, 2]] if K.shape == (3, 3) else [float(v) for v in K.reshape(-1)[:4]]


def _pose_record(p) -> Pose:
    if isinstance(p, Pose):
        return p
    if isinstance(p, Pose3D):
        return p.to_record()
    rec = Pose()
    rec.pose[:] = np.asarray(p, dtype=np.float64).reshape(16).tolist()
    return rec


def _params(cls, defaults: str, params, what: Optional[str] = None):
    """``params`` as a ``cls`` record: itself, or the C defaults (``lib().<defaults>``) with a dict's fields set over them.
    With ``what`` (the record's name in words) a key that is no field of the record (a misspelt name) is an error, not ignored"""
    if isinstance(params, cls):
        return params
    if what is not None and isinstance(params, dict):
        unknown = sorted(set(params) - {f for f, _ in cls._fields_})
        if unknown:
            raise PPFError(_capi.PPF_ERR_INVALID, f"unknown {what} parameter(s): {', '.join(unknown)}")
    prm = cls()
    getattr(lib(), defaults)(C.byref(prm))
    for key, v in (params or {}).items():
        setattr(prm, key, v)
    return prm


def _depth_image(depth, error: str):
    """(the contiguous float32 image, rows, cols) of a 2-D depth image; anything else raises ``error``"""
    img = np.ascontiguousarray(depth, dtype=np.float32) if depth is not None else None
    if img is None or img.ndim != 2:
        raise PPFError(_capi.PPF_ERR_INVALID, error)
    return (img,) + img.shape


_DEPTH_FORMATS = {np.dtype(np.float32): _capi.PPF_DEPTH_F32, np.dtype(np.uint16): _capi.PPF_DEPTH_U16}   # by numpy dtype
_NO_DEVICE = contextlib.nullcontext()


@functools.lru_cache(maxsize=None)
def _torch_formats():
    """(torch, PPF_DEPTH_* by torch dtype): torch is only imported once a tensor has come in"""
    import torch
    return torch, {torch.float32: _capi.PPF_DEPTH_F32, torch.uint16: _capi.PPF_DEPTH_U16}


def _depth_params(depth_scale, z_min, z_max, flags: int = 0) -> _capi.DepthParams:
    dp = _capi.DepthParams()
    lib().ppf_default_depth_params(C.byref(dp))
    dp.depth_scale, dp.z_min, dp.z_max, dp.flags = float(depth_scale), float(z_min), float(z_max), flags
    return dp


class _DepthInput:
    """A depth image as the entries take it: ``ptr``, ``rows``, ``cols``, ``pitch`` (bytes) and ``format`` of ``keep``, the
    array or tensor they point into.  ``is_device``: a GPU tensor, for the ``*_device`` entry, called inside ``device()`` with
    ``stream()``; otherwise a numpy array (a CPU tensor goes the numpy way) for the host entry."""

    __slots__ = ("keep", "ptr", "rows", "cols", "shape", "pitch", "format", "is_device", "torch")

    def __init__(self, depth, error: str, shape=None, dtype=None):
        """shape and dtype (a numpy dtype): what the image must have, None for any 2-D float32 or uint16 image; error: the text
        for a wrong dtype, rank or shape, formatted only when raised, with ``{kind}`` ("tensor" or "array"), ``{shape}`` and
        ``{dtype}``.  Rows are read at their stride; an image whose strides are not row strides is copied."""
        is_torch = type(depth).__module__.startswith("torch")
        self.is_device = is_torch and depth.is_cuda
        if self.is_device:
            self.torch, formats = _torch_formats()
        else:
            depth, formats = np.asarray(depth.numpy() if is_torch else depth), _DEPTH_FORMATS
        self.format = formats.get(depth.dtype)
        self.shape = tuple(depth.shape)
        if (self.format is None or len(self.shape) != 2 or (shape is not None and self.shape != tuple(shape))
                or (dtype is not None and self.format != _DEPTH_FORMATS[dtype])):
            raise PPFError(_capi.PPF_ERR_INVALID, error.format(kind="tensor" if self.is_device else "array", shape=shape, dtype=dtype))
        self.rows, self.cols = self.shape
        if self.is_device:
            if depth.stride(1) != 1 or depth.stride(0) < self.cols:
                depth = depth.contiguous()
            self.ptr, self.pitch = C.c_void_p(depth.data_ptr()), depth.stride(0) * depth.element_size()
        else:
            size, (pitch, step) = depth.itemsize, depth.strides
            if step != size or pitch < self.cols * size or pitch % size:
                depth = np.ascontiguousarray(depth)
                pitch = depth.strides[0]
            self.ptr, self.pitch = C.c_void_p(depth.ctypes.data), pitch
        self.keep = depth

    def device(self):
        """the context the entry is called in: the tensor's device made current, nothing for a host image"""
        return self.torch.cuda.device(self.keep.device) if self.is_device else _NO_DEVICE

    def stream(self):
        """the ``stream`` argument of the device entry: the tensor's device's current stream, None for stream 0"""
        stream = self.torch.cuda.current_stream(self.keep.device).cuda_stream
        return C.c_void_p(stream) if stream else None

    def output(self, out, dtype, shape=None, tensor_error: Optional[str] = None):
        """(out, its pointer): ``out`` checked, or made when None -- a contiguous image of ``dtype`` (a numpy scalar type) and
        ``shape`` (None: the input's) where the entry writes: a tensor on the input's device for a GPU input, a writeable
        numpy array otherwise.  tensor_error: another text for a refused tensor, ``{shape}`` filled in when raised"""
        shape = self.shape if shape is None else tuple(shape)
        if self.is_device:
            torch = self.torch
            want = getattr(torch, dtype.__name__)
            if out is None:
                out = torch.empty(shape, dtype=want, device=self.keep.device)
            elif not (getattr(out, "is_cuda", False) and out.device == self.keep.device and out.dtype == want
                      and tuple(out.shape) == shape and out.is_contiguous()):
                raise PPFError(_capi.PPF_ERR_INVALID, (tensor_error or "out must be a contiguous {dtype} tensor of shape {shape} on the "
                                                       "depth image's device").format(dtype=dtype.__name__, shape=shape))
            return out, C.c_void_p(out.data_ptr())
        if out is None:
            out = np.empty(shape, dtype)
        elif not (isinstance(out, np.ndarray) and out.dtype == dtype and out.shape == shape and out.flags.c_contiguous
                  and out.flags.writeable):
            raise PPFError(_capi.PPF_ERR_INVALID, f"out must be a contiguous {dtype.__name__} array of shape {shape}")
        return out, C.c_void_p(out.ctypes.data)


def _frame_tables(dets, poses, top):
    """the FrameDetection, Pose and count arrays of one call: dets[i] is (model cloud, object cloud) or None"""
    n = len(dets)
    if len(poses) != n:
        raise PPFError(_capi.PPF_ERR_INVALID, f"{len(poses)} pose lists for {n} detections")
    counts = [len(p) if d is not None else 0 for d, p in zip(dets, poses)]
    top = int(top) if top is not None else max([1] + counts)
    arr = (FrameDetection * max(n, 1))()
    recs = (Pose * (max(n, 1) * top))()
    n_poses = (C.c_int * max(n, 1))()
    for i, (d, plist) in enumerate(zip(dets, poses)):
        if d is None:
            continue
        arr[i].model_cloud = d[0]._ptr
        if d[1] is not None:
            arr[i].scene = d[1]._ptr
        n_poses[i] = len(plist)
        for k, p in enumerate(plist[:top]):
            recs[i * top + k] = _pose_record(p)
    return n, top, arr, recs, n_poses


def _verify_call(entry, tables, img, rows, cols, it, *prms):
    """either verify entry on the tables of _frame_tables: (scores (n_dets, top), best (n_dets,), the counters)"""
    n, top, arr, recs, n_poses = tables
    scores = (PoseScore * (max(n, 1) * top))()
    best = (C.c_int * max(n, 1))()
    st = VerifyStats()
    check(entry(arr, n, recs, n_poses, top, img.ctypes.data if img is not None else None, rows, cols, it, *[C.byref(p) for p in prms],
                scores, best, C.byref(st)))
    out = np.ctypeslib.as_array(scores).copy()[:n * top].reshape(n, top)
    return out, np.array(best[:n], dtype=np.int32), _capi.stats_dict(st)


def verify_frame(dets, poses, top: Optional[int] = None, depth=None, intr=None, params=None):
    """One ppf_verify_frame call: score every pose of every detection against its object cloud and, when ``depth`` is given,
    against the depth image.  dets: per detection a (model cloud, object cloud) pair of DeviceClouds, or
    None; poses: per detection its poses (Pose3D, Pose records or 4x4 arrays), at most ``top`` of them (default: the
    longest list).  depth: a 2-D float32 image in metres or None; intr: (fx, fy, ppx, ppy) or the 3x3 camera matrix.
    params: a VerifyParams, a dict of its fields (the rest default) or None.  Returns (scores, best, stats): the
    PoseScore rows as a numpy structured array of shape (n_dets, top) (rows past a detection's poses are zero), the best
    index per detection (-1 without poses) and the call's counters as a dict."""
    tables = _frame_tables(dets, poses, top)
    prm = _params(VerifyParams, "ppf_default_verify_params", params)
    img, it, rows, cols = None, None, 0, 0
    if depth is not None:
        img, rows, cols = _depth_image(depth, "depth must be a 2-D float32 image")
        it = (C.c_double * 4)(*_intr4(intr))
    return _verify_call(lib().ppf_verify_frame, tables, img, rows, cols, it, prm)


def verify_frame_rendered(dets, poses, top: Optional[int] = None, depth=None, intr=None, params=None, render_params=None,
                          image_size=None):
    """One ppf_verify_frame_rendered call: verify_frame, with a model row considered only where it is visible in a surfel
    z-buffer of its own pose.  The render needs the image: ``image_size`` (rows, cols) and ``intr`` are
    required when ``depth`` is None, and default to the depth image's size otherwise.  render_params: a RenderParams, a
    dict of its fields (the rest default) or None.  Returns (scores, best, stats) as verify_frame does."""
    tables = _frame_tables(dets, poses, top)
    prm = _params(VerifyParams, "ppf_default_verify_params", params)
    rprm = _params(RenderParams, "ppf_default_render_params", render_params)
    img = None
    if depth is not None:
        img, rows, cols = _depth_image(depth, "depth must be a 2-D float32 image")
        if image_size is not None and tuple(image_size) != img.shape:
            raise PPFError(_capi.PPF_ERR_INVALID, f"image_size {tuple(image_size)} is not the depth image's {img.shape}")
    elif image_size is not None:
        rows, cols = (int(v) for v in image_size)
    else:
        raise PPFError(_capi.PPF_ERR_INVALID, "verify_frame_rendered needs a depth image or image_size")
    it = (C.c_double * 4)(*_intr4(intr)) if intr is not None else None
    return _verify_call(lib().ppf_verify_frame_rendered, tables, img, rows, cols, it, prm, rprm)


def render_frame(dets, poses, which, rows: int, cols: int, intr, render_params=None, top: Optional[int] = None, return_stats: bool = False):
    """One ppf_render_frame call: pose ``which[i]`` of detection i (skipped where -1 or where dets[i] is None) drawn as
    surfel disks into one rows x cols z-buffer.  dets: per detection a model cloud (DeviceCloud), a
    (model cloud, anything) pair, or None; poses: per detection its poses as verify_frame takes them; which: the
    ``best`` of either verify entry plugs in.  Returns (depth, label): float32 metres with 0 where empty and int32
    detection indices with -1 where empty; with ``return_stats`` also the call's counters."""
    pairs = [None if d is None else (d[0] if isinstance(d, tuple) else d, None) for d in dets]
    n, top, arr, recs, _ = _frame_tables(pairs, poses, top)
    if len(which) != n:
        raise PPFError(_capi.PPF_ERR_INVALID, f"{len(which)} entries of which for {n} detections")
    ws = (C.c_int * max(n, 1))(*[int(w) if pairs[i] is not None else -1 for i, w in enumerate(which)])
    rprm = _params(RenderParams, "ppf_default_render_params", render_params)
    it = (C.c_double * 4)(*_intr4(intr)) if intr is not None else None
    depth = np.zeros((max(int(rows), 0), max(int(cols), 0)), dtype=np.float32)
    label = np.full(depth.shape, -1, dtype=np.int32)
    st = RenderStats()
    check(lib().ppf_render_frame(arr, n, recs, ws, top, int(rows), int(cols), it, C.byref(rprm), depth.ctypes.data, label.ctypes.data,
                                 C.byref(st)))
    return (depth, label, _capi.stats_dict(st)) if return_stats else (depth, label)


def select_frame(dets, poses, depth, intr, params=None, render_params=None, scores=None, top: Optional[int] = None,
                 return_images: bool = False, return_stats: bool = False):
    """One ppf_select_frame call: one consistent set among all poses of all detections of a frame.  dets:
    per detection a model cloud (DeviceCloud), a (model cloud, anything) pair, or None; poses: per detection its poses as
    verify_frame takes them; depth: the 2-D float32 image in metres (required); intr: (fx, fy, ppx, ppy) or the 3x3 camera
    matrix.  params: a SelectParams, a dict of its fields (the rest default) or None; render_params as render_frame takes
    them.  scores: the (n_dets, top) PoseScore rows of either verify entry, whose ``score`` then ranks the hypotheses, or
    None to rank by the explained share.  Returns (info, selected): the SelectInfo rows as a numpy structured array of shape
    (n_dets, top) and the selected flat indices i * top + k in selection order; with ``return_images`` also the depth
    (0 where empty) and label (flat index, -1 where empty) images of the selection, with ``return_stats`` the counters."""
    pairs = [None if d is None else (d[0] if isinstance(d, tuple) else d, None) for d in dets]
    n, top, arr, recs, n_poses = _frame_tables(pairs, poses, top)
    prm = _params(SelectParams, "ppf_default_select_params", params)
    rprm = _params(RenderParams, "ppf_default_render_params", render_params)
    img, rows, cols = _depth_image(depth, "select_frame needs a 2-D float32 depth image")
    it = (C.c_double * 4)(*_intr4(intr)) if intr is not None else None
    sc = None
    if scores is not None:
        given = np.ascontiguousarray(scores)
        if given.shape != (n, top) or given.dtype.itemsize != C.sizeof(PoseScore):
            raise PPFError(_capi.PPF_ERR_INVALID, f"scores must be the ({n}, {top}) PoseScore rows of a verify call")
        sc = (PoseScore * (max(n, 1) * top)).from_buffer_copy(given.tobytes() + bytes(C.sizeof(PoseScore) * (top if n == 0 else 0)))
    info = (SelectInfo * (max(n, 1) * top))()
    selected = (C.c_int * (max(n, 1) * top))()
    n_selected = C.c_int(0)
    out_d = np.zeros((rows, cols), dtype=np.float32) if return_images else None
    out_l = np.full((rows, cols), -1, dtype=np.int32) if return_images else None
    st = SelectStats()
    check(lib().ppf_select_frame(arr, n, recs, n_poses, top, sc, img.ctypes.data, rows, cols, it, C.byref(rprm), C.byref(prm), info, selected,
                                 C.byref(n_selected), out_d.ctypes.data if return_images else None,
                                 out_l.ctypes.data if return_images else None, C.byref(st)))
    out = [np.ctypeslib.as_array(info).copy()[:n * top].reshape(n, top), np.array(selected[:n_selected.value], dtype=np.int32)]
    if return_images:
        out += [out_d, out_l]
    if return_stats:
        out.append(_capi.stats_dict(st))
    return tuple(out)


def refine_frame(dets, poses, depth, intr, params=None, top: Optional[int] = None, return_stats: bool = False):
    """One ppf_refine_frame call: every pose of every detection refined on the depth image itself by projective
    point-to-plane steps -- to polish the poses select_frame kept at full depth resolution, or to carry the
    poses of the last frame into this frame's depth image without matching again.  dets: per detection a model cloud
    (DeviceCloud), a (model cloud, anything) pair, or None; poses: per detection its poses as verify_frame takes them;
    depth: the 2-D float32 image in metres (required); intr: (fx, fy, ppx, ppy) or the 3x3 camera matrix.  params: a
    RefineParams, a dict of its fields (the rest default) or None.  Returns (refined, info): per detection the list of its
    refined poses (Pose3D) and the RefineInfo rows as a numpy structured array of shape (n_dets, top); with
    ``return_stats`` also the call's counters."""
    pairs = [None if d is None else (d[0] if isinstance(d, tuple) else d, None) for d in dets]
    n, top, arr, recs, n_poses = _frame_tables(pairs, poses, top)
    prm = _params(RefineParams, "ppf_default_refine_params", params)
    img, rows, cols = _depth_image(depth, "refine_frame needs a 2-D float32 depth image")
    it = (C.c_double * 4)(*_intr4(intr)) if intr is not None else None
    out = (Pose * (max(n, 1) * top))()
    info = (RefineInfo * (max(n, 1) * top))()
    st = RefineStats()
    check(lib().ppf_refine_frame(arr, n, recs, n_poses, top, img.ctypes.data, rows, cols, it, C.byref(prm), out, info, C.byref(st)))
    refined = [[Pose3D(out[i * top + k]) for k in range(n_poses[i])] for i in range(n)]
    rows_info = np.ctypeslib.as_array(info).copy()[:n * top].reshape(n, top)
    return (refined, rows_info, _capi.stats_dict(st)) if return_stats else (refined, rows_info)


def camera(cam) -> _capi.Camera:
    """A ``ppf_camera`` record from: a Camera; (fx, fy, cx, cy) or a 3x3 camera matrix (pinhole); a dict of its fields; or any
    object with those attributes (fx, fy, cx, cy and optionally k1..k6, p1, p2, max_r)."""
    if isinstance(cam, _capi.Camera):
        return cam
    names = [f for f, _ in _capi.Camera._fields_ if f != "reserved"]
    c = _capi.Camera()
    if isinstance(cam, dict) or hasattr(cam, "fx"):
        get = cam.get if isinstance(cam, dict) else (lambda k, d=0.0: getattr(cam, k, d))
        lib().ppf_default_camera(C.byref(c), float(get("fx")), float(get("fy")), float(get("cx")), float(get("cy")))
        for f in names[4:]:
            setattr(c, f, float(get(f, 0.0)))
        return c
    lib().ppf_default_camera(C.byref(c), *_intr4(cam))
    return c


def camera_points(cam, pts, unproject: bool = False):
    """ppf_camera_project (normalised points -> pixels) or, with ``unproject``, ppf_camera_unproject (pixels -> normalised
    points) of an (n, 2) array, on the host: (points (n, 2) float64, NaN where invalid; valid (n,) bool)."""
    a = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
    out = np.empty_like(a)
    valid = np.zeros(a.shape[0], np.uint8)
    fn = lib().ppf_camera_unproject if unproject else lib().ppf_camera_project
    check(fn(C.byref(camera(cam)), a.ctypes.data, a.shape[0], out.ctypes.data, valid.ctypes.data))
    return out, valid.astype(bool)


def map_boxes(cam_from, cam_to, to_rows: int, to_cols: int, boxes) -> np.ndarray:
    """ppf_camera_map_boxes: the boxes (x, y, w, h) of a detector run on the raw colour image (camera ``cam_from``, with its
    distortion) carried into the pinhole camera ``cam_to`` the aligned depth image lives in; (n, 4) int32, a box that
    cannot be mapped is all zero."""
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
    out = np.zeros_like(b)
    check(lib().ppf_camera_map_boxes(C.byref(camera(cam_from)), C.byref(camera(cam_to)), int(to_rows), int(to_cols), b.ctypes.data,
                                     b.shape[0], out.ctypes.data))
    return out


class DepthMap:
    """A resident registration map (``ppf_depth_map``): built once per calibration from the depth camera, the colour camera
    and the extrinsics (R, t: depth frame -> colour frame, metres); ``register`` then aligns each raw depth frame to the
    colour camera's pixel grid on the device."""

    def __init__(self, depth_cam, depth_shape, color_cam, color_shape, R, t):
        self.depth_shape = (int(depth_shape[0]), int(depth_shape[1]))
        self.color_shape = (int(color_shape[0]), int(color_shape[1]))
        self.color_cam = camera(color_cam)
        R9 = np.ascontiguousarray(R, dtype=np.float64).reshape(-1)
        t3 = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
        if R9.size != 9 or t3.size != 3:
            raise PPFError(_capi.PPF_ERR_INVALID, "R must have 9 elements and t 3")
        self._ptr = C.c_void_p()
        check(lib().ppf_depth_map_create(C.byref(camera(depth_cam)), self.depth_shape[0], self.depth_shape[1], C.byref(self.color_cam),
                                         self.color_shape[0], self.color_shape[1], R9.ctypes.data, t3.ctypes.data, C.byref(self._ptr)))

    def __del__(self):
        try:
            if self._ptr:
                lib().ppf_depth_map_release(self._ptr)
                self._ptr = None
        except Exception:
            pass

    @property
    def intr(self):
        """(fx, fy, ppx, ppy) of the aligned image: what every later stage takes"""
        c = self.color_cam
        return (c.fx, c.fy, c.cx, c.cy)

    def rays(self) -> np.ndarray:
        """the ray table, (rows, cols, 2) float64, NaN NaN where a depth pixel has no ray"""
        out = np.empty(self.depth_shape + (2,), np.float64)
        check(lib().ppf_depth_map_rays(self._ptr, out.ctypes.data))
        return out

    def register(self, depth, *, depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0, params=None, out=None,
                 return_stats: bool = False):
        """The depth frame drawn into the colour camera's pixel grid (ppf_depth_register): float32 metres, 0 where nothing
        was drawn.  depth: a 2-D numpy float32 (metres) or uint16 (units of depth_scale metres) array of the map's depth
        size, rows read at its stride, which gives a numpy image; or such a torch tensor on the GPU, read in place on
        ``torch.cuda.current_stream()`` (ppf_depth_register_device), which gives a float32 tensor on the same device (or
        fills ``out``).  params: a RegisterParams, a dict of its fields or None (the defaults)."""
        prm = _params(_capi.RegisterParams, "ppf_default_register_params", params)
        dp = _depth_params(depth_scale, z_min, z_max)
        st = _capi.RegisterStats()
        inp = _DepthInput(depth, "depth must be a float32 or uint16 {kind} of shape {shape}", shape=self.depth_shape)
        dp.format = inp.format
        # a host image always gets a fresh numpy image
        out, optr = inp.output(out if inp.is_device else None, np.float32, self.color_shape,
                               "out must be a contiguous float32 GPU tensor of shape {shape}")
        with inp.device():
            if inp.is_device:
                check(lib().ppf_depth_register_device(self._ptr, inp.ptr, inp.pitch, C.byref(dp), C.byref(prm), optr, inp.stream(), C.byref(st)))
            else:
                check(lib().ppf_depth_register(self._ptr, inp.ptr, inp.pitch, C.byref(dp), C.byref(prm), optr, C.byref(st)))
        return (out, _capi.stats_dict(st)) if return_stats else out


def filter_depth(depth, *, depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0, params=None, out=None,
                 return_stats: bool = False):
    """The depth image without its unsupported ("flying") pixels and smoothed inside each surface (ppf_depth_filter,
    DESIGN.md §23): float32 metres of the same shape, 0 where nothing is written -- what ``DeviceCloud.from_depth``,
    ``DepthMap.register`` and the frame stages take.  depth: a 2-D numpy float32 (metres) or uint16 (units of depth_scale
    metres) array, rows read at its stride, which gives a numpy image; or such a torch tensor on the GPU, read in place on
    ``torch.cuda.current_stream()`` (ppf_depth_filter_device), which gives a float32 tensor on the same device (or fills
    ``out``, which must not overlap the input).  params: a DepthFilterParams, a dict of its fields or None (the defaults)."""
    prm = _params(_capi.DepthFilterParams, "ppf_default_depth_filter_params", params, "depth filter")
    dp = _depth_params(depth_scale, z_min, z_max)
    st = _capi.DepthFilterStats()
    inp = _DepthInput(depth, "depth must be a 2-D float32 or uint16 {kind}")
    dp.format = inp.format
    out, optr = inp.output(out, np.float32)
    with inp.device():
        if inp.is_device:
            check(lib().ppf_depth_filter_device(inp.ptr, inp.rows, inp.cols, inp.pitch, C.byref(dp), C.byref(prm), optr, inp.stream(), C.byref(st)))
        else:
            check(lib().ppf_depth_filter(inp.ptr, inp.rows, inp.cols, inp.pitch, C.byref(dp), C.byref(prm), optr, C.byref(st)))
    return (out, _capi.stats_dict(st)) if return_stats else out


class DepthHistory:
    """The last ``window`` depth images of a fixed camera, resident on the device, and the image they fuse into
    (ppf_depth_history): ``push`` takes a frame and gives the fused float32 image -- less noise, the holes of
    this frame filled from the frames before it, flickering pixels gone -- that ``filter_depth``, ``DeviceCloud.from_depth``
    and the frame stages take.  shape: (rows, cols) of every frame; dtype: numpy float32 (metres) or uint16 (units of
    depth_scale metres), fixed like the shape; params: a DepthHistoryParams, a dict of its fields (window, range_abs,
    range_quad, min_support, max_age, flags) or None (the defaults)."""

    def __init__(self, shape, *, dtype=np.float32, depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0, params=None):
        self._ptr = None
        self.params = _params(_capi.DepthHistoryParams, "ppf_default_depth_history_params", params, "depth history")
        fmt = _DEPTH_FORMATS.get(np.dtype(dtype))
        if fmt is None or len(tuple(shape)) != 2:
            raise PPFError(_capi.PPF_ERR_INVALID, "a depth history takes a (rows, cols) shape and float32 or uint16 frames")
        self.shape = (int(shape[0]), int(shape[1]))
        self.dtype = np.dtype(dtype)
        dp = _depth_params(depth_scale, z_min, z_max)
        dp.format = fmt
        ptr = C.c_void_p()
        check(lib().ppf_depth_history_create(self.shape[0], self.shape[1], C.byref(dp), C.byref(self.params), C.byref(ptr)))
        self._ptr = ptr

    def __del__(self):
        try:
            if self._ptr is not None:
                lib().ppf_depth_history_release(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def reset(self) -> None:
        """forget every frame: the next push sees no older one"""
        check(lib().ppf_depth_history_reset(self._ptr))

    def info(self) -> dict:
        """rows, cols, window, frames (pushes since the last reset) and device_bytes"""
        d = _capi.DepthHistoryDesc()
        check(lib().ppf_depth_history_info(self._ptr, C.byref(d)))
        return {k: v for k, v in _capi.stats_dict(d).items() if not k.startswith("reserved")}

    def push(self, depth, out=None, return_state: bool = False, return_stats: bool = False):
        """Push one frame and get the fused image (float32 metres, 0 where nothing is written).  depth: a 2-D numpy array of
        the history's shape and dtype, rows read at its stride, which gives a numpy image; or such a torch tensor on the GPU,
        read in place on ``torch.cuda.current_stream()`` (ppf_depth_history_push_device), which gives a float32 tensor on the
        same device (or fills ``out``, which must not overlap the input).  return_state adds the uint8 state image (0 empty,
        1 measured, 2 filled, 3 unsupported, +16 changed), return_stats the counters: (image[, state][, stats])."""
        st = _capi.DepthHistoryStats()
        inp = _DepthInput(depth, "depth must be a {dtype} {kind} of shape {shape}", shape=self.shape, dtype=self.dtype)
        out, optr = inp.output(out, np.float32)
        state, sptr = inp.output(None, np.uint8) if return_state else (None, None)
        with inp.device():
            if inp.is_device:
                check(lib().ppf_depth_history_push_device(self._ptr, inp.ptr, inp.pitch, optr, sptr, inp.stream(), C.byref(st)))
            else:
                check(lib().ppf_depth_history_push(self._ptr, inp.ptr, inp.pitch, optr, sptr, C.byref(st)))
        res = (out,) + ((state,) if return_state else ()) + ((_capi.stats_dict(st),) if return_stats else ())
        return res if len(res) > 1 else out


# ppf_depth_motion_level as a numpy record
MOTION_LEVEL = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("rows", "<i4"), ("cols", "<i4"), ("n_source", "<i4"),
                         ("n_pairs_first", "<i4"), ("n_pairs_last", "<i4"), ("rmse_first", "<f4"), ("rmse_last", "<f4"),
                         ("reserved", "<i4", 3)])


def depth_motion(prev, cur, intr, *, depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0, params=None, init=None,
                 return_info: bool = False, return_stats: bool = False):
    """The camera's rigid motion between two depth images (ppf_depth_motion): the 4 x 4 float64 ``T`` with
    ``p_cur = T p_prev`` for a static point, so a pose (model -> camera) of the previous frame is ``T @ pose`` in the current
    one.  prev, cur: two 2-D images of one shape and dtype, numpy float32 (metres) or uint16 (units of depth_scale metres),
    rows read at their strides; or two such torch tensors on one GPU, read in place on ``torch.cuda.current_stream()``
    (ppf_depth_motion_device).  intr: (fx, fy, ppx, ppy) or the 3x3 camera matrix.  params: a DepthMotionParams, a dict of its
    fields (``iters`` a sequence of up to four counts, level 0 first) or None (the defaults); init: a 4 x 4 start, default the
    identity.  return_info adds the four level rows (MOTION_LEVEL records, level 0 first), return_stats the call's counters;
    ``stats["status"]`` LOST or STEP means the motion was not found and ``T`` is the start."""
    if isinstance(params, dict) and "iters" in params:
        params = dict(params)
        iters = [int(v) for v in params.pop("iters")]
        if len(iters) > _capi.PPF_MOTION_MAX_LEVELS:
            raise PPFError(_capi.PPF_ERR_INVALID, f"iters holds more than {_capi.PPF_MOTION_MAX_LEVELS} levels")
        prm = _params(_capi.DepthMotionParams, "ppf_default_depth_motion_params", params, "depth motion")
        for l, v in enumerate(iters):
            prm.iters[l] = v
    else:
        prm = _params(_capi.DepthMotionParams, "ppf_default_depth_motion_params", params, "depth motion")
    a = _DepthInput(prev, "prev must be a 2-D float32 or uint16 {kind}")
    b = _DepthInput(cur, "cur must be a {dtype} {kind} of shape {shape}, as prev is", shape=a.shape,
                    dtype=next(d for d, f in _DEPTH_FORMATS.items() if f == a.format))
    if a.is_device != b.is_device or (a.is_device and a.keep.device != b.keep.device):
        raise PPFError(_capi.PPF_ERR_INVALID, "prev and cur must both be numpy arrays or both be tensors on one GPU")
    dp = _depth_params(depth_scale, z_min, z_max)
    dp.format = a.format
    it = (C.c_double * 4)(*_intr4(intr))
    start = None
    if init is not None:
        m = np.ascontiguousarray(init, dtype=np.float64)
        if m.size != 16:
            raise PPFError(_capi.PPF_ERR_INVALID, "init must be a 4 x 4 matrix")
        start = (C.c_double * 16)(*m.reshape(-1).tolist())
    pose = (C.c_double * 16)()
    rows = (_capi.DepthMotionLevel * _capi.PPF_MOTION_MAX_LEVELS)()
    st = _capi.DepthMotionStats()
    with a.device():
        if a.is_device:
            check(lib().ppf_depth_motion_device(a.ptr, a.pitch, b.ptr, b.pitch, a.rows, a.cols, it, C.byref(dp), C.byref(prm), start, a.stream(),
                                                pose, rows, C.byref(st)))
        else:
            check(lib().ppf_depth_motion(a.ptr, a.pitch, b.ptr, b.pitch, a.rows, a.cols, it, C.byref(dp), C.byref(prm), start, pose, rows,
                                         C.byref(st)))
    T = np.array(pose, dtype=np.float64).reshape(4, 4)
    res = (T,) + ((np.frombuffer(bytes(rows), dtype=MOTION_LEVEL).copy(),) if return_info else ()) + \
        ((_capi.stats_dict(st),) if return_stats else ())
    return res if len(res) > 1 else T


def _mat44_mul(A, B) -> np.ndarray:
    """A B as ppf_mat44_mul adds it up (0 + a0 b0 + a1 b1 + a2 b2 + a3 b3, nothing fused): the same bytes on every machine"""
    A, B = np.asarray(A, dtype=np.float64).reshape(4, 4).tolist(), np.asarray(B, dtype=np.float64).reshape(4, 4).tolist()
    out = np.empty((4, 4), np.float64)
    for i in range(4):
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc = acc + A[i][k] * B[k][j]
            out[i, j] = acc
    return out


def _pose_premultiply(p: Pose3D, T) -> None:
    """p.pose <- T p.pose, with t, q and angle of the new matrix"""
    M = _mat44_mul(T, p.pose)
    R = M[:3, :3]
    p.pose, p.t = M, M[:3, 3].copy()
    p.angle = float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    w = np.sqrt(max(0.0, 1.0 + np.trace(R))) / 2.0
    if w > 1e-6:
        q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    else:  # a half turn: the axis from the diagonal
        ax = np.sqrt(np.maximum(0.0, (np.diag(R) + 1.0) / 2.0))
        q = np.array([0.0, ax[0], np.copysign(ax[1], R[0, 1]), np.copysign(ax[2], R[0, 2])])
    p.q = q / np.linalg.norm(q)


class DepthOdometry:
    """Frame-to-frame camera tracking on depth images alone: ``push`` takes the next frame, runs ``depth_motion`` from the
    frame kept before it and accumulates ``pose``, which takes the first frame's camera coordinates to the current frame's.
    rows, cols, intr: fixed for the stream; depth_scale, z_min, z_max, params: as ``depth_motion`` takes them.  A numpy frame
    is copied, a GPU tensor is cloned on its device, so the caller may reuse its buffer."""

    def __init__(self, rows: int, cols: int, intr, *, depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0, params=None):
        self.shape = (int(rows), int(cols))
        self.intr = _intr4(intr)
        self._kw = dict(depth_scale=depth_scale, z_min=z_min, z_max=z_max, params=params)
        self.reset()

    def reset(self) -> None:
        """forget the previous frame; ``pose`` is the identity again and the next push only keeps its frame"""
        self._prev = None
        self.pose = np.eye(4)
        self.frames = 0
        self.last_info = None
        self.last_stats: Dict[str, object] = {}

    def push(self, depth, keep_on_failure: bool = False):
        """(T, status): the motion from the frame kept before to this one and PPF_MOTION_* of the call; the first push gives
        the identity and PPF_MOTION_NONE.  On LOST or STEP ``pose`` stays where it was, T is the identity, and the new frame
        becomes the next previous frame only with ``keep_on_failure`` (else the next push is measured against the old one)."""
        if tuple(depth.shape) != self.shape:
            raise PPFError(_capi.PPF_ERR_INVALID, f"depth must have the shape {self.shape}")
        own = depth.clone() if type(depth).__module__.startswith("torch") else np.array(depth)
        if self._prev is None:
            self._prev = own
            self.frames = 1
            return np.eye(4), _capi.PPF_MOTION_NONE
        T, self.last_info, self.last_stats = depth_motion(self._prev, own, self.intr, return_info=True, return_stats=True, **self._kw)
        status = int(self.last_stats["status"])
        failed = status in (_capi.PPF_MOTION_LOST, _capi.PPF_MOTION_STEP)
        if failed:
            T = np.eye(4)
        else:
            self.pose = _mat44_mul(T, self.pose)
        if not failed or keep_on_failure:
            self._prev = own
        self.frames += 1
        return T, status


# ppf_depth_volume_voxel as a numpy record
VOLUME_VOXEL = np.dtype([("d", "<f4"), ("w", "<i4")])


def _pose16(pose):
    m = np.ascontiguousarray(pose, dtype=np.float64)
    if m.size != 16:
        raise PPFError(_capi.PPF_ERR_INVALID, "pose must be a 4 x 4 matrix")
    return (C.c_double * 16)(*m.reshape(-1).tolist())


class DepthVolume:
    """A truncated signed distance volume on the device that posed depth images are fused into (ppf_depth_volume, DESIGN.md
    §30): ``integrate`` adds a frame seen from a pose, ``raycast`` gives the model depth image from any pose -- a float32
    image every depth stage takes, the denoised and hole-filled frame of a moving camera, and with ``depth_motion`` the
    drift-free frame-to-model tracking of ``DepthFusion`` -- and ``extract`` the zero surface as a ``DeviceCloud`` with normals,
    which ``PPF3DDetector.trainModel`` takes.  dims: (nx, ny, nz); voxel: metres; origin: world coordinates of the centre of
    voxel (0, 0, 0); trunc: metres, None: 4 voxels; a pose is a 4 x 4 world -> camera matrix, as ``DepthOdometry.pose`` is."""

    def __init__(self, dims, voxel: float, origin, trunc: Optional[float] = None, max_weight: int = 64):
        self._ptr = None
        prm = _capi.DepthVolumeParams()
        lib().ppf_default_depth_volume_params(C.byref(prm))
        dims, origin = [int(v) for v in dims], [float(v) for v in origin]
        if len(dims) != 3 or len(origin) != 3:
            raise PPFError(_capi.PPF_ERR_INVALID, "a depth volume takes dims (nx, ny, nz) and an origin (x, y, z)")
        prm.dims[:], prm.origin[:] = dims, origin
        prm.voxel = float(voxel)
        prm.trunc = float(np.float32(4) * np.float32(voxel)) if trunc is None else float(trunc)
        prm.max_weight = int(max_weight)
        self.params = prm
        ptr = C.c_void_p()
        check(lib().ppf_depth_volume_create(C.byref(prm), C.byref(ptr)))
        self._ptr = ptr
        self.dims = tuple(dims)

    def __del__(self):
        try:
            if self._ptr is not None:
                lib().ppf_depth_volume_release(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def reset(self) -> None:
        """every voxel unobserved again"""
        check(lib().ppf_depth_volume_reset(self._ptr))

    def info(self) -> dict:
        """dims, voxel, origin, trunc, max_weight, integrations (since the last reset) and device_bytes"""
        d = _capi.DepthVolumeDesc()
        check(lib().ppf_depth_volume_info(self._ptr, C.byref(d)))
        out = {k: v for k, v in _capi.stats_dict(d).items() if not k.startswith("reserved")}
        out["dims"], out["origin"] = tuple(d.dims), tuple(d.origin)
        return out

    def read(self):
        """(d float32, w int32), each of shape (nz, ny, nx): a blocking copy of every voxel"""
        nx, ny, nz = self.dims
        rec = np.empty(nx * ny * nz, VOLUME_VOXEL)
        check(lib().ppf_depth_volume_read(self._ptr, rec.ctypes.data, rec.size))
        return rec["d"].reshape(nz, ny, nx).copy(), rec["w"].reshape(nz, ny, nx).copy()

    def integrate(self, depth, intr, pose, *, depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0,
                  return_stats: bool = False):
        """Fuse one frame seen from ``pose``.  depth: a 2-D numpy float32 (metres) or uint16 (units of depth_scale metres)
        array, rows read at its stride; or such a torch tensor on the GPU, read in place on ``torch.cuda.current_stream()``
        (ppf_depth_volume_integrate_device).  intr: (fx, fy, ppx, ppy) or the 3x3 camera matrix.  Returns the number of
        voxels updated, or the call's counters with return_stats."""
        inp = _DepthInput(depth, "depth must be a 2-D float32 or uint16 {kind}")
        dp = _depth_params(depth_scale, z_min, z_max)
        dp.format = inp.format
        it, T, st = (C.c_double * 4)(*_intr4(intr)), _pose16(pose), _capi.DepthVolumeIntegrateStats()
        with inp.device():
            if inp.is_device:
                check(lib().ppf_depth_volume_integrate_device(self._ptr, inp.ptr, inp.rows, inp.cols, inp.pitch, it, C.byref(dp), T,
                                                              inp.stream(), C.byref(st)))
            else:
                check(lib().ppf_depth_volume_integrate(self._ptr, inp.ptr, inp.rows, inp.cols, inp.pitch, it, C.byref(dp), T, C.byref(st)))
        return _capi.stats_dict(st) if return_stats else int(st.n_updated)

    def raycast(self, shape, intr, pose, params=None, out=None, return_normals: bool = False, return_stats: bool = False):
        """The volume's depth image (float32 metres, 0 where no surface is hit) of ``shape`` = (rows, cols) seen through
        ``intr`` from ``pose``; neither needs to be an input's.  params: a DepthVolumeRaycastParams, a dict of its fields
        (z_near, z_far, ray_step, min_weight) or None.  out: None (a new numpy image), a contiguous float32 numpy array of
        that shape, or such a torch tensor on the GPU, which is written in place on ``torch.cuda.current_stream()``
        (ppf_depth_volume_raycast_device) and makes the normals a tensor too.  return_normals adds the (rows, cols, 3) normals
        in camera coordinates (zeros where there is none), return_stats the counters: (image[, normals][, stats])."""
        prm = _params(_capi.DepthVolumeRaycastParams, "ppf_default_depth_volume_raycast_params", params, "depth volume raycast")
        shape = (int(shape[0]), int(shape[1]))
        it, T, st = (C.c_double * 4)(*_intr4(intr)), _pose16(pose), _capi.DepthVolumeRaycastStats()
        on_device = type(out).__module__.startswith("torch") and out.is_cuda
        if on_device:
            torch, _ = _torch_formats()
            if not (out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()):
                raise PPFError(_capi.PPF_ERR_INVALID, f"out must be a contiguous float32 tensor of shape {shape}")
            nrm = torch.empty(shape + (3,), dtype=torch.float32, device=out.device) if return_normals else None
            stream = torch.cuda.current_stream(out.device).cuda_stream
            with torch.cuda.device(out.device):
                check(lib().ppf_depth_volume_raycast_device(self._ptr, shape[0], shape[1], it, T, C.byref(prm), C.c_void_p(out.data_ptr()),
                                                            C.c_void_p(nrm.data_ptr()) if return_normals else None,
                                                            C.c_void_p(stream) if stream else None, C.byref(st)))
        else:
            if out is None:
                out = np.empty(shape, np.float32)
            elif not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == shape and out.flags.c_contiguous
                      and out.flags.writeable):
                raise PPFError(_capi.PPF_ERR_INVALID, f"out must be a contiguous float32 array of shape {shape}")
            nrm = np.empty(shape + (3,), np.float32) if return_normals else None
            check(lib().ppf_depth_volume_raycast(self._ptr, shape[0], shape[1], it, T, C.byref(prm), out.ctypes.data,
                                                 nrm.ctypes.data if return_normals else None, C.byref(st)))
        res = (out,) + ((nrm,) if return_normals else ()) + ((_capi.stats_dict(st),) if return_stats else ())
        return res if len(res) > 1 else out

    def extract(self, params=None, return_stats: bool = False):
        """The zero surface as a ``DeviceCloud``: rows x y z nx ny nz in world coordinates, one per sign change between two
        observed neighbours that has a normal.  params: a DepthVolumeExtractParams, a dict (min_weight) or None."""
        prm = _params(_capi.DepthVolumeExtractParams, "ppf_default_depth_volume_extract_params", params, "depth volume extract")
        out, st = C.c_void_p(), _capi.DepthVolumeExtractStats()
        check(lib().ppf_depth_volume_extract(self._ptr, C.byref(prm), C.byref(out), C.byref(st)))
        cloud = DeviceCloud(out)
        return (cloud, _capi.stats_dict(st)) if return_stats else cloud


    def write(self, d, w) -> None:
        """The inverse of ``read``: d float32 and w int32 of shape (nz, ny, nx) (or flat, in linear order) replace every voxel
        (ppf_depth_volume_write): a saved scan restored.  w must lie in 0 .. max_weight and d be finite in [-1, 1]."""
        nx, ny, nz = self.dims
        d, w = np.asarray(d), np.asarray(w)
        if d.size != nx * ny * nz or w.size != d.size:
            raise PPFError(_capi.PPF_ERR_INVALID, f"write takes d and w of {nx * ny * nz} voxels each")
        rec = np.empty(d.size, VOLUME_VOXEL)
        rec["d"], rec["w"] = d.reshape(-1), w.reshape(-1)
        check(lib().ppf_depth_volume_write(self._ptr, rec.ctypes.data, rec.size))

    def mesh(self, params=None, return_stats: bool = False):
        """The zero surface as a ``VolumeMesh``: a triangle mesh by marching tetrahedra over the cubes whose eight voxels are
        all observed and unsaturated (ppf_depth_volume_mesh).  params: a DepthVolumeMeshParams, a dict
        (min_weight) or None."""
        prm = _params(_capi.DepthVolumeMeshParams, "ppf_default_depth_volume_mesh_params", params, "depth volume mesh")
        out, st = C.c_void_p(), _capi.DepthVolumeMeshStats()
        check(lib().ppf_depth_volume_mesh(self._ptr, C.byref(prm), C.byref(out), C.byref(st)))
        m = VolumeMesh(out)
        return (m, _capi.stats_dict(st)) if return_stats else m


class VolumeMesh:
    """The triangle mesh ``DepthVolume.mesh`` made, resident on the device (ppf_volume_mesh): vertices are rows
    x y z nx ny nz in world coordinates, triangles three vertex indices each, counter-clockwise seen from free space."""

    def __init__(self, ptr):
        self._ptr = ptr
        d = _capi.VolumeMeshDesc()
        check(lib().ppf_volume_mesh_info(self._ptr, C.byref(d)))
        self.n_vertices, self.n_triangles, self.device_bytes = int(d.n_vertices), int(d.n_triangles), int(d.device_bytes)
        self._host = None

    def __del__(self):
        try:
            if self._ptr is not None:
                lib().ppf_volume_mesh_release(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def _read(self):
        if self._host is None:
            v, t = np.empty((self.n_vertices, 6), np.float32), np.empty((self.n_triangles, 3), np.int32)
            check(lib().ppf_volume_mesh_read(self._ptr, v.ctypes.data if v.size else None, self.n_vertices,
                                             t.ctypes.data if t.size else None, self.n_triangles))
            self._host = (v, t)
        return self._host

    def vertices(self) -> np.ndarray:
        """(N, 6) float32: x y z nx ny nz; a normal of 0 0 0 where the volume gives none"""
        return self._read()[0].copy()

    def triangles(self) -> np.ndarray:
        """(M, 3) int32 vertex indices"""
        return self._read()[1].copy()

    def save_ply(self, path) -> None:
        """an ASCII PLY that ``ply.load_ply_mesh`` and ``CloudProcessor.LoadMeshModel`` read"""
        from .ply import write_ply_mesh
        v, t = self._read()
        write_ply_mesh(v, t, path)

    @classmethod
    def from_arrays(cls, vertices, triangles) -> "VolumeMesh":
        """A mesh from host arrays (ppf_volume_mesh_upload), so that a loaded PLY can be cleaned by ``components``: vertices
        (N, 3) float32, or (N, >= 6) with the normals in the last three columns; triangles (M, 3) int32."""
        V = np.ascontiguousarray(vertices, dtype=np.float32)
        T = np.ascontiguousarray(triangles, dtype=np.int32)
        if V.size == 0:
            V = V.reshape(0, 3)
        if T.size == 0:
            T = T.reshape(0, 3)
        if V.ndim != 2 or T.ndim != 2 or T.shape[1] != 3 or V.shape[1] in (4, 5):
            raise PPFError(_capi.PPF_ERR_INVALID, "from_arrays: vertices must be (N, 3 | >= 6) float32 and triangles (M, 3) int32")
        out = C.c_void_p()
        check(lib().ppf_volume_mesh_upload(V.ctypes.data if V.size else None, V.shape[0], max(V.shape[1], 3),
                                           V.shape[1] - 3 if V.shape[1] >= 6 else -1, T.ctypes.data if T.size else None, T.shape[0],
                                           C.byref(out)))
        return cls(out)

    def components(self, min_triangles: int = 1, min_area: float = 0.0, rank_lo: int = 0, rank_hi: Optional[int] = None, *,
                   labels: bool = False, max_info: int = 64, return_stats: bool = False, measure_only: bool = False):
        """The mesh's connected components, ranked by area, and the mesh of those that are kept
        (ppf_volume_mesh_components): a component is kept iff rank_lo <= rank < rank_hi (None: no upper end),
        it has at least min_triangles triangles and at least min_area square metres.  Returns (VolumeMesh, [info dicts of the
        max_info largest components]), then the per-vertex labels (rank, or -1) with labels=True, then the stats with
        return_stats=True.  measure_only: no output mesh is made and the first item is None.  This mesh is not changed."""
        prm = _params(_capi.MeshComponentParams, "ppf_default_mesh_component_params",
                      {"min_triangles": int(min_triangles), "min_area": float(min_area), "rank_lo": int(rank_lo),
                       "rank_hi": 0x7FFFFFFF if rank_hi is None else int(rank_hi)})
        cap = int(max_info)
        info = (_capi.MeshComponentInfo * max(cap, 1))()
        lab = np.empty(self.n_vertices, np.int32) if labels else None
        out, st = C.c_void_p(), _capi.MeshComponentStats()
        check(lib().ppf_volume_mesh_components(self._ptr, C.byref(prm), None if measure_only else C.byref(out),
                                               lab.ctypes.data if lab is not None and lab.size else None, info if cap > 0 else None, cap,
                                               C.byref(st)))
        res = [None if measure_only else VolumeMesh(out),
               [_component_info(info[r]) for r in range(min(int(st.n_components), max(cap, 0)))]]
        if labels:
            res.append(lab)
        if return_stats:
            res.append(_capi.stats_dict(st))
        return tuple(res)

    def largest(self, k: int = 1, **kw):
        """``components`` keeping the k largest pieces (rank_hi = k) among those that pass min_triangles and min_area"""
        return self.components(rank_lo=0, rank_hi=int(k), **kw)

    def split(self, k: int, **kw) -> list:
        """The k largest pieces, one ``VolumeMesh`` each (rank_lo = r, rank_hi = r + 1; a rank that fails min_triangles or
        min_area gives an empty mesh).  Fewer than k when the mesh has fewer components."""
        kw = {key: v for key, v in kw.items() if key in ("min_triangles", "min_area")}
        pieces = []
        for r in range(int(k)):
            m, _, st = self.components(rank_lo=r, rank_hi=r + 1, max_info=0, return_stats=True, **kw)
            if r >= st["n_components"]:
                break
            pieces.append(m)
        return pieces


def _component_info(rec) -> dict:
    """a ppf_mesh_component_info as a plain dict (lo / hi as tuples)"""
    d = {name: getattr(rec, name) for name, _ in rec._fields_ if name != "reserved"}
    d["lo"], d["hi"] = tuple(rec.lo), tuple(rec.hi)
    return d


class DepthFusion:
    """Frame-to-model camera tracking and fusion: every pushed frame is aligned to the image ``volume`` gives from the current
    ``pose`` (``depth_motion(prev = raycast, cur = frame)``), which does not accumulate drift as ``DepthOdometry``'s chain does,
    and is then integrated at the new pose.  rows, cols, intr: fixed for the stream; volume: a ``DepthVolume``, whose world is
    the first frame's camera; motion_params, raycast_params: as ``depth_motion`` and ``DepthVolume.raycast`` take them;
    depth_scale, z_min, z_max: the frames'.  A uint16 frame is tracked as float32 metres, z = (float)((double)d * depth_scale)."""

    def __init__(self, rows: int, cols: int, intr, volume: DepthVolume, *, motion_params=None, raycast_params=None,
                 depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0):
        self.shape = (int(rows), int(cols))
        self.intr = _intr4(intr)
        self.volume = volume
        self.motion_params, self.raycast_params = motion_params, raycast_params
        self._kw = dict(depth_scale=depth_scale, z_min=z_min, z_max=z_max)
        self.pose = np.eye(4)
        self.frames = 0
        self.model_depth = None
        self.last_info = None
        self.last_stats: Dict[str, object] = {}

    def _metres(self, depth):
        is_torch = type(depth).__module__.startswith("torch")
        if is_torch:
            torch, _ = _torch_formats()
            return depth if depth.dtype == torch.float32 else (depth.to(torch.float64) * self._kw["depth_scale"]).to(torch.float32)
        depth = np.asarray(depth)
        return depth if depth.dtype == np.float32 else (depth.astype(np.float64) * np.float64(self._kw["depth_scale"])).astype(np.float32)

    def push(self, depth):
        """(T, status): the motion from the model's image to this frame and PPF_MOTION_* of the call; the first push
        integrates at the identity and gives the identity and PPF_MOTION_NONE.  On LOST or STEP ``pose`` and the volume stay
        as they were and T is the identity."""
        if tuple(depth.shape) != self.shape:
            raise PPFError(_capi.PPF_ERR_INVALID, f"depth must have the shape {self.shape}")
        if self.frames == 0:
            self.volume.integrate(depth, self.intr, self.pose, **self._kw)
            self.frames = 1
            return np.eye(4), _capi.PPF_MOTION_NONE
        cur = self._metres(depth)
        on_device = type(cur).__module__.startswith("torch") and cur.is_cuda
        out = _torch_formats()[0].empty(self.shape, dtype=cur.dtype, device=cur.device) if on_device else None
        self.model_depth = self.volume.raycast(self.shape, self.intr, self.pose, params=self.raycast_params, out=out)
        T, self.last_info, self.last_stats = depth_motion(self.model_depth, cur, self.intr, z_min=self._kw["z_min"], z_max=self._kw["z_max"],
                                                          params=self.motion_params, return_info=True, return_stats=True)
        status = int(self.last_stats["status"])
        self.frames += 1
        if status in (_capi.PPF_MOTION_LOST, _capi.PPF_MOTION_STEP):
            return np.eye(4), status
        self.pose = _mat44_mul(T, self.pose)
        self.volume.integrate(depth, self.intr, self.pose, **self._kw)
        return T, status


# ppf_segment_info as a numpy record
SEGMENT_INFO =np.dtype([("n_pixels", "<i4"), ("n_border", "<i4"), ("first_pixel", "<i4"), ("box_xywh", "<i4", 4), ("z_lo", "<f4"),
                         ("z_hi", "<f4"), ("reserved", "<i4", 3)])


def segment_depth(depth, *, depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0, normals=None, params=None,
                  out=None, return_info: bool = False, return_stats: bool = False):
    """The depth image's connected surfaces, labelled in image space (ppf_depth_segments): an int32 image of
    the same shape holding each pixel's segment rank (largest segment 0) or -1.  Two adjacent kept pixels are linked iff
    their depths differ by at most ``depth_abs + depth_quad * Zp * Zq`` and -- with ``normals``, the DeviceCloud that
    ``DeviceCloud.from_depth(depth, ..., normals={...})`` gives for this image (no ``drop``) -- both are smooth (curvature
    <= ``curvature_threshold``) and their normals agree (``normal_cos``); the other pixels with a normal join the nearest
    smooth neighbour in depth.  depth: a 2-D numpy float32 (metres) or uint16 (units of depth_scale metres) array, rows read
    at its stride, which gives a numpy image; or such a torch tensor on the GPU, read in place on
    ``torch.cuda.current_stream()`` (ppf_depth_segments_device), which gives an int32 tensor on the same device (or fills
    ``out``, which must not overlap the input).  params: a SegmentParams, a dict of its fields or None (the defaults).
    return_info adds the segments' ``SEGMENT_INFO`` records (one per segment) and the counts (segments, valid components,
    all components); return_stats adds the call's stats last."""
    prm = _params(_capi.SegmentParams, "ppf_default_segment_params", params, "segment")
    dp = _depth_params(depth_scale, z_min, z_max)
    if normals is not None and not isinstance(normals, DeviceCloud):
        raise PPFError(_capi.PPF_ERR_INVALID, "normals must be a DeviceCloud or None")
    nrm = normals._ptr if normals is not None else None
    mc = max(1, min(int(prm.max_segments), _capi.PPF_CLUSTER_MAX_CLUSTERS))
    info = np.zeros(mc, dtype=SEGMENT_INFO)
    counts = np.zeros(3, dtype=np.int32)
    st = _capi.SegmentStats()
    tail = (info.ctypes.data_as(C.POINTER(_capi.SegmentInfo)), counts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st))

    def result(labels):
        res = [labels]
        if return_info:
            res += [info[:int(counts[0])].copy(), counts]
        if return_stats:
            res.append(_capi.stats_dict(st))
        return labels if len(res) == 1 else tuple(res)

    inp = _DepthInput(depth, "depth must be a 2-D float32 or uint16 {kind}")
    dp.format = inp.format
    out, optr = inp.output(out, np.int32)
    with inp.device():
        if inp.is_device:
            check(lib().ppf_depth_segments_device(inp.ptr, inp.rows, inp.cols, inp.pitch, C.byref(dp), nrm, C.byref(prm), optr, inp.stream(), *tail))
        else:
            check(lib().ppf_depth_segments(inp.ptr, inp.rows, inp.cols, inp.pitch, C.byref(dp), nrm, C.byref(prm), optr, *tail))
    return result(out)


def depth_edges(depth, intr=None, *, depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0, fp64: bool = False,
                normals=None, params=None, cloud: bool = False, out=None, return_stats: bool = False):
    """Where the depth image says a surface ends (ppf_depth_edges): a uint8 image of the same shape whose bits
    are PPF_EDGE_OCCLUDING (the near side of a depth step of more than ``depth_abs + depth_quad * Zp * Zq``, looked for in 8
    directions across up to ``max_gap`` unmeasured pixels), PPF_EDGE_OCCLUDED (the far side), PPF_EDGE_BOUNDARY (unmeasured
    pixels with nothing behind them) and -- with ``normals``, the DeviceCloud that ``DeviceCloud.from_depth(depth, ...,
    normals={...})`` gives for this image (no ``drop``) -- PPF_EDGE_CURVATURE (curvature > ``curvature_threshold``).  With
    ``cloud=True`` also the edge cloud, a DeviceCloud of the pixels whose mask meets ``select`` in row-major order, which
    ``Matching_S2B`` and the frame stages take: the normals cloud's rows with normals, else ``x y z 0 0 0`` from ``intr``
    ((fx, fy, ppx, ppy) or the 3x3 matrix; ``fp64`` as in ``from_depth``).  depth: a 2-D numpy float32 (metres) or uint16
    (units of depth_scale metres) array, rows read at its stride, which gives a numpy mask; or such a torch tensor on the
    GPU, read in place on ``torch.cuda.current_stream()`` (ppf_depth_edges_device), which gives a uint8 tensor on the same
    device (or fills ``out``, which must not overlap the input).  params: a DepthEdgeParams, a dict of its fields or None
    (the defaults).  Returns the mask, then the cloud with ``cloud``, then the stats with ``return_stats``."""
    prm = _params(_capi.DepthEdgeParams, "ppf_default_depth_edge_params", params, "depth edge")
    dp = _depth_params(depth_scale, z_min, z_max, _capi.PPF_DEPTH_FP64 if fp64 else 0)
    if normals is not None and not isinstance(normals, DeviceCloud):
        raise PPFError(_capi.PPF_ERR_INVALID, "normals must be a DeviceCloud or None")
    nrm = normals._ptr if normals is not None else None
    it = (C.c_double * 4)(*_intr4(intr)) if intr is not None else None
    st = _capi.DepthEdgeStats()
    found = C.c_void_p()
    inp = _DepthInput(depth, "depth must be a 2-D float32 or uint16 {kind}")
    dp.format = inp.format
    out, optr = inp.output(out, np.uint8)
    tail = (C.byref(found) if cloud else None, C.byref(st))
    with inp.device():
        if inp.is_device:
            check(lib().ppf_depth_edges_device(inp.ptr, inp.rows, inp.cols, inp.pitch, it, C.byref(dp), nrm, C.byref(prm), optr, inp.stream(), *tail))
        else:
            check(lib().ppf_depth_edges(inp.ptr, inp.rows, inp.cols, inp.pitch, it, C.byref(dp), nrm, C.byref(prm), optr, *tail))
    res = [out] + ([DeviceCloud(found)] if cloud else []) + ([_capi.stats_dict(st)] if return_stats else [])
    return out if len(res) == 1 else tuple(res)


# ppf_recognize_score as a numpy record
RECOGNIZE_SCORE = np.dtype([("model", "<i4"), ("reserved", "<i4"), ("n_known", "<u8"), ("n_keys_hit", "<u8"), ("precision", "<f8"),
                            ("recall", "<f8"), ("score", "<f8")])


class Recognizer:
    """Which trained models a proposal cloud can be a view of (ppf_recognizer_*, ppf_recognize_frame): every
    model's set of quantised pair-feature keys, built once on the device.  models: trained ``PPF3DDetector``s (feature 0,
    either key_equality); the recogniser keeps their tables alive."""

    def __init__(self, models: Sequence[PPF3DDetector]):
        models = list(models)
        for d in models:
            if not isinstance(d, PPF3DDetector) or not d.trained:
                raise PPFError(_capi.PPF_ERR_NOT_TRAINED, "Recognizer takes trained PPF3DDetector objects")
        self._ptr = None
        self.n_models = len(models)
        ptrs = (C.c_void_p * max(len(models), 1))(*[d._model.ptr for d in models])
        out = C.c_void_p()
        check(lib().ppf_recognizer_create(ptrs, len(models), C.byref(out)))
        self._ptr = out

    def __del__(self):
        try:
            if self._ptr:
                lib().ppf_recognizer_release(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def model_info(self, i: int) -> dict:
        """n_rows, n_bins (n_a, n_a, n_a, n_d), in_lds, n_keys and bytes of model i's key set"""
        ri = _capi.RecognizerInfo()
        check(lib().ppf_recognizer_model_info(self._ptr, int(i), C.byref(ri)))
        d = _capi.stats_dict(ri)
        d.pop("reserved")
        return d

    def keys(self, i: int) -> np.ndarray:
        """model i's key set: (n_keys, 4) int32 tuples in lexicographic order"""
        n = C.c_int(0)
        lib().ppf_recognizer_keys(self._ptr, int(i), None, 0, C.byref(n))  # PPF_ERR_CAPACITY: n is the size
        out = np.zeros((max(n.value, 1), 4), dtype=np.int32)
        check(lib().ppf_recognizer_keys(self._ptr, int(i), out.ctypes.data, out.shape[0], C.byref(n)))
        return out[:n.value]

    def recognize(self, clouds, params=None, return_counts: bool = False, return_stats: bool = False):
        """Per cloud (a ``DeviceCloud`` or None) its candidates, best first: a ``RECOGNIZE_SCORE`` array of at most ``top``
        rows.  params: a RecognizeParams, a dict of its fields (max_rows, top, min_score, min_precision) or None (the
        defaults).  return_counts adds ``n_used`` (n_clouds) and ``counts`` (n_clouds, n_models, 2: n_known, n_keys_hit);
        return_stats adds the call's stats last."""
        prm = _params(_capi.RecognizeParams, "ppf_default_recognize_params", params, "recognize")
        clouds = list(clouds)
        for c in clouds:
            if c is not None and not isinstance(c, DeviceCloud):
                raise PPFError(_capi.PPF_ERR_INVALID, "clouds must be DeviceCloud objects or None")
        n = len(clouds)
        ptrs = (C.c_void_p * max(n, 1))(*[c._ptr if c is not None else None for c in clouds])
        top = max(1, min(int(prm.top), _capi.PPF_RECOGNIZE_MAX_TOP))
        ranked = np.zeros((max(n, 1), top), dtype=RECOGNIZE_SCORE)
        n_ranked = np.zeros(max(n, 1), dtype=np.int32)
        n_used = np.zeros(max(n, 1), dtype=np.int32)
        counts = np.zeros((max(n, 1), self.n_models, 2), dtype=np.uint64)
        st = _capi.RecognizeStats()
        check(lib().ppf_recognize_frame(self._ptr, ptrs, n, C.byref(prm), n_used.ctypes.data, counts.ctypes.data,
                                        ranked.ctypes.data_as(C.POINTER(_capi.RecognizeScore)),
                                        n_ranked.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(st)))
        res = [[ranked[i, :int(n_ranked[i])].copy() for i in range(n)]]
        if return_counts:
            res += [n_used[:n], counts[:n]]
        if return_stats:
            res.append(_capi.stats_dict(st))
        return res[0] if len(res) == 1 else tuple(res)


class CloudProcessor:
    """``ppf::CloudProcessor``: holds the scene cloud, the depth image, the detector's boxes, the per-object clouds
    and the PPF detectors; every method is the reference's, in the order its driver calls them
    (src/YOLO_cropping_ppf_test.cpp:84-123)."""

    def __init__(self, scene: Optional[np.ndarray] = None, depth: Optional[np.ndarray] = None,
                 boxes: Sequence[Sequence[int]] = (), classIds: Sequence[int] = (), indices: Sequence[int] = (),
                 relativeSamplingStep: float = 0.025, relativeDistanceStep: float = 0.05):
        self.scene = DeviceCloud.upload(scene) if scene is not None else None
        self.depth = None if depth is None else np.ascontiguousarray(depth, dtype=np.float32)
        self.boxes, self.classIds, self.indices = [tuple(b) for b in boxes], list(classIds), list(indices)
        self.relativeSamplingStep, self.relativeDistanceStep = relativeSamplingStep, relativeDistanceStep
        self.objects: List[DeviceCloud] = []
        self.objects_with_normals: List[DeviceCloud] = []
        self.objects_edges: List[DeviceCloud] = []
        self.models: List[np.ndarray] = []
        self.detectors: List[PPF3DDetector] = []
        self.if_trained: List[bool] = []
        self.label_to_id: Dict[str, int] = {}
        self.id_to_label: Dict[int, str] = {}
        self._model_clouds: Dict[int, DeviceCloud] = {}
        self.timings: Dict[str, float] = {}  # seconds spent in the last resident match / ICP call
        # PrepareFrame: one resident to-Mat (object, edge) pair per detection, rows per stage per detection
        self.object_mats: List[DeviceCloud] = []
        self.edge_mats: List[DeviceCloud] = []
        self.stage_rows: Optional[np.ndarray] = None
        self.frame_stats: Dict[str, object] = {}
        self.match_frame_stats: Dict[str, float] = {}  # ppf_match_frame counters of the last MatchFrame (summed over its calls)
        self.frame_intr: Optional[tuple] = None  # PrepareFrame's (fx, fy, ppx, ppy)
        # MatchFrame: per detection its refined top poses in match rank order, and the labels it was called with
        self.frame_poses: List[List[Pose3D]] = []
        self.frame_labels: List[Optional[str]] = []
        # PoseValidation: the score rows (n_dets, top), the best index per detection, the call's counters
        self.pose_scores: Optional[np.ndarray] = None
        self.best_index: List[int] = []
        self.verify_stats: Dict[str, object] = {}
        self.kept_index: List[int] = []  # per detection the pose PoseValidation kept, -1 where it kept none
        self.render_stats: Dict[str, object] = {}  # RenderFrame: the ppf_render_frame counters
        # SelectFrame: the info rows (n_dets, top), the selected (detection, k) pairs in selection order, the counters
        self.select_info: Optional[np.ndarray] = None
        self.selected: List[tuple] = []
        self.select_stats: Dict[str, object] = {}
        # RefineFrame: the info rows (n_dets, top) and the counters
        self.refine_info: Optional[np.ndarray] = None
        self.refine_stats: Dict[str, object] = {}
        self._last_refined: List[Pose3D] = []
        # RemovePlanes: the info rows of the planes taken out of the scene, and the counters
        self.plane_info: Optional[np.ndarray] = None
        self.plane_stats: Dict[str, object] = {}
        # ProposeBoxes: the info rows of the scene's clusters, and the counters
        self.cluster_info: Optional[np.ndarray] = None
        self.cluster_stats: Dict[str, object] = {}
        self.depth_filter_stats: Dict[str, object] = {}  # FilterDepth: the ppf_depth_filter counters
        # FuseDepth: the ppf_depth_history counters and state image of the last frame, and the history with what it was made for
        self.depth_history_stats: Dict[str, object] = {}
        self.depth_state = None
        self._depth_history: Optional[tuple] = None
        # TrackCamera: the last motion, its level rows and the ppf_depth_motion counters
        self.camera_motion: Optional[np.ndarray] = None
        self.motion_info = None
        self.motion_stats: Dict[str, object] = {}
        # FuseVolume: the DepthFusion the processor owns and its fused world -> camera pose
        self._depth_fusion: Optional[DepthFusion] = None
        self.camera_pose: Optional[np.ndarray] = None
        # ProposeSegments: the info rows of the image's segments, its label image and the counters
        self.segment_info: Optional[np.ndarray] = None
        self.segment_labels: Optional[np.ndarray] = None
        self.segment_stats: Dict[str, object] = {}
        self._depth_normals_of: tuple = (None, None)  # the (scene, depth) pair Deprojection(normals=...) last made
        # EdgeExtractionDepth: the edge mask of the depth image and the ppf_depth_edges counters
        self.depth_edge_mask: Optional[np.ndarray] = None
        self.depth_edge_stats: Dict[str, object] = {}
        # RecognizeFrame: per detection its (label, score, precision, recall) candidates, best first, and the counters
        self.frame_candidates: List[List[tuple]] = []
        self.recognize_stats: Dict[str, object] = {}
        self._recognizer: Optional[tuple] = None  # (the detectors' model handles, their Recognizer)

    # ---- the PCL half -------------------------------------------------------------------------------------
    def Deprojection(self, CameraIntr, fp64: bool = False, normals: Optional[dict] = None) -> DeviceCloud:
        """The scene cloud from ``self.depth`` (float32 metres), back-projected on the device -- the reference's
        ``Deprojection(Mat CameraIntr)`` is an empty stub (CloudProcessing.h:262).  CameraIntr: the 3x3 matrix as
        SceneCropping takes it.  Sets and returns ``self.scene``; fp64 and normals as in ``DeviceCloud.from_depth``."""
        if self.depth is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "Deprojection needs a depth image")
        self.scene = DeviceCloud.from_depth(self.depth, np.asarray(CameraIntr, dtype=np.float64), fp64=fp64, normals=normals)
        self._depth_normals_of = (self.scene, self.depth) if normals is not None and not normals.get("drop", False) else (None, None)
        return self.scene

    def FilterDepth(self, params=None) -> np.ndarray:
        """``self.depth`` without its unsupported pixels and smoothed inside each surface (``filter_depth``), the step in
        front of Deprojection.  params: the fields of ppf_depth_filter_params (radius, range_abs, range_quad, support_abs,
        support_quad, min_support).  Sets ``depth_filter_stats``; replaces and returns ``self.depth``."""
        if self.depth is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "FilterDepth needs a depth image")
        self.depth, self.depth_filter_stats = filter_depth(self.depth, params=params, return_stats=True)
        return self.depth

    def FuseDepth(self, depth, params=None):
        """The next frame of a fixed camera fused with the frames before it (``DepthHistory.push``): less noise, this frame's
        holes filled, flicker gone.  depth: the new frame, as ``DepthHistory.push`` takes it; params: the fields of
        ppf_depth_history_params (window, range_abs, range_quad, min_support, max_age, flags).  The processor keeps one
        history; it starts afresh when the frame's shape, dtype or the parameters change.  Sets ``self.depth`` to the fused
        image, ``depth_history_stats`` and ``depth_state`` (the uint8 state image); returns the fused image, so FilterDepth /
        Deprojection follow as on a single frame."""
        if depth is None or not hasattr(depth, "shape") or len(depth.shape) != 2:
            raise PPFError(_capi.PPF_ERR_INVALID, "FuseDepth needs a 2-D depth image")
        prm = _params(_capi.DepthHistoryParams, "ppf_default_depth_history_params", params, "depth history")
        dtype = np.dtype(str(depth.dtype).replace("torch.", ""))
        key = (tuple(depth.shape), dtype, bytes(prm))
        if self._depth_history is None or self._depth_history[0] != key:
            self._depth_history = (key, DepthHistory(tuple(depth.shape), dtype=dtype, params=prm))
        self.depth, self.depth_state, self.depth_history_stats = self._depth_history[1].push(depth, return_state=True, return_stats=True)
        return self.depth

    def RemovePlanes(self, **params) -> DeviceCloud:
        """``self.scene`` without its support planes (ppf_prep_planes), the step before SceneCropping / PrepareFrame: a
        box's corners lie on the background, so without it every object cloud is mostly table.  params: the fields of
        ppf_plane_params (distance_threshold, n_hypotheses, seed, max_planes, min_inliers, min_inlier_share, flags).
        Sets ``plane_info`` (the info rows) and ``plane_stats``; replaces and returns ``self.scene``."""
        if self.scene is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "RemovePlanes needs a scene cloud")
        self.scene, self.plane_info, self.plane_stats = self.scene.remove_planes(params, return_info=True)
        return self.scene

    def ProposeBoxes(self, CameraIntr, params=None) -> List[DeviceCloud]:
        """Detections without a detector: ``self.scene`` -- plane-free, so after RemovePlanes -- split into its object
        clusters (ppf_prep_clusters) and ``self.boxes`` set to the clusters' image boxes, largest cluster first, so that
        PrepareFrame / MatchFrame run on a bare depth frame.  CameraIntr: the 3x3 matrix as SceneCropping takes it; the
        image is ``self.depth``'s.  params: the fields of ppf_cluster_params (tolerance, min_size, max_size, max_clusters).
        Sets ``cluster_info`` (one row per cluster) and ``cluster_stats``; returns the cluster clouds."""
        if self.scene is None or self.depth is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "ProposeBoxes needs a scene cloud and a depth image")
        found, info, counts, self.cluster_stats = self.scene.clusters(params, np.asarray(CameraIntr, dtype=np.float64), self.depth.shape,
                                                                      return_info=True)
        self.cluster_info = info[:int(counts[0])].copy()
        self.boxes = [tuple(int(v) for v in row["box_xywh"]) for row in self.cluster_info]
        return found

    def ProposeRegions(self, CameraIntr, params=None) -> List[DeviceCloud]:
        """ProposeBoxes for objects that touch: ``self.scene`` -- with normals and curvature, as ``Deprojection(normals=...)``
        leaves it -- split into its smooth surface regions (ppf_prep_regions) and ``self.boxes`` set to the regions' image
        boxes, largest region first.  params: the fields of ppf_region_params (tolerance, normal_cos, curvature_threshold,
        min_size, max_size, max_regions, flags).  Sets ``cluster_info`` (one row per region) and ``cluster_stats``; returns
        the region clouds."""
        if self.scene is None or self.depth is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "ProposeRegions needs a scene cloud and a depth image")
        found, info, counts, self.cluster_stats = self.scene.regions(params, np.asarray(CameraIntr, dtype=np.float64), self.depth.shape,
                                                                     return_info=True)
        self.cluster_info = info[:int(counts[0])].copy()
        self.boxes = [tuple(int(v) for v in row["box_xywh"]) for row in self.cluster_info]
        return found

    def ProposeSegments(self, params=None) -> np.ndarray:
        """ProposeBoxes without leaving the image: ``self.depth`` split into its connected surfaces in image space
        (``segment_depth``, ppf_depth_segments) and ``self.boxes`` set to the segments' boxes, largest segment first.  When
        ``self.scene`` is what ``Deprojection(normals=...)`` gave for this depth image it serves as the normals cloud;
        otherwise depth alone decides.  params: the fields of ppf_segment_params (depth_abs, depth_quad, normal_cos,
        curvature_threshold, min_size, max_size, max_segments, flags).  Sets ``segment_info`` (one row per segment),
        ``segment_labels`` and ``segment_stats``; returns the label image."""
        if self.depth is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "ProposeSegments needs a depth image")
        made = self.scene is not None and self.scene is self._depth_normals_of[0] and self.depth is self._depth_normals_of[1]
        normals = self.scene if made else None
        self.segment_labels, self.segment_info, _, self.segment_stats = segment_depth(self.depth, normals=normals, params=params,
                                                                                      return_info=True, return_stats=True)
        self.boxes = [tuple(int(v) for v in row["box_xywh"]) for row in self.segment_info]
        return self.segment_labels

    def SceneCropping(self, CameraIntr) -> List[DeviceCloud]:
        """CameraIntr: 3x3 matrix (fx, fy on the diagonal, ppx, ppy in the last column), as the reference passes it"""
        K = np.asarray(CameraIntr, dtype=np.float64)
        intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        for box in self.boxes:
            self.objects.append(self.scene.crop(box, self.depth, intr))
        return self.objects

    def Subsampling(self, leafsize: float) -> List[DeviceCloud]:
        self.objects = [o.voxel_grid(leafsize) for o in self.objects]
        return self.objects

    def OutlierProcessing(self, meanK: int = 50, Thresh: float = 1.5) -> List[DeviceCloud]:
        self.objects = [o.outlier_removal(meanK, Thresh) for o in self.objects]
        return self.objects

    def NormalEstimation(self, k: int = 30) -> List[DeviceCloud]:
        self.objects_with_normals += [o.normals(k) for o in self.objects]
        return self.objects_with_normals

    def EdgeExtraction(self, curvThreshold: float) -> List[DeviceCloud]:
        self.objects_edges += [o.edges(curvThreshold) for o in self.objects_with_normals]
        return self.objects_edges

    def EdgeExtractionDepth(self, params=None, CameraIntr=None) -> DeviceCloud:
        """EdgeExtraction for the depth route: the edge cloud of ``self.depth`` itself (``depth_edges``, ppf_depth_edges) --
        its occluding and boundary pixels, which the curvature of depth normals never marks.  When ``self.scene`` is what
        ``Deprojection(normals=...)`` gave for this depth image it serves as the normals cloud, so the rows carry its normals
        and the curvature edges join; otherwise the rows are ``x y z 0 0 0`` and CameraIntr (the 3x3 matrix) is needed.
        params: the fields of ppf_depth_edge_params (depth_abs, depth_quad, max_gap, curvature_threshold, select).  Sets
        ``depth_edge_mask`` and ``depth_edge_stats``; appends the cloud to ``objects_edges``, where EdgeExtraction leaves the
        clouds that Matching_S2B takes as ``edge``, and returns it."""
        if self.depth is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "EdgeExtractionDepth needs a depth image")
        made = self.scene is not None and self.scene is self._depth_normals_of[0] and self.depth is self._depth_normals_of[1]
        intr = None if CameraIntr is None else np.asarray(CameraIntr, dtype=np.float64)
        self.depth_edge_mask, edge, self.depth_edge_stats = depth_edges(self.depth, intr, normals=self.scene if made else None,
                                                                        params=params, cloud=True, return_stats=True)
        self.objects_edges.append(edge)
        return edge

    @staticmethod
    def PointCloudXYZNormalToMat(pcl_cloud: DeviceCloud, resident: bool = False):
        """the N x 6 Mat of the reference (numpy array); ``resident=True`` keeps it on the device (a DeviceCloud that
        Matching / Matching_S2B accept directly, so no cloud crosses PCIe between the crop and the pose)"""
        mat = pcl_cloud.to_mat()
        return mat if resident else mat.rows()

    def PrepareFrame(self, CameraIntr, leafsize: float = 0.003, meanK: int = 50, Thresh: float = 1.0, k: int = 30,
                     curvThreshold: float = 0.03) -> List[tuple]:
        """SceneCropping -> Subsampling -> OutlierProcessing -> NormalEstimation -> EdgeExtraction ->
        PointCloudXYZNormalToMat for every box at once (one ppf_prep_frame call instead of a loop per box and stage).
        Fills ``object_mats`` / ``edge_mats`` (device-resident, what MatchFrame consumes) and ``stage_rows``."""
        K = np.asarray(CameraIntr, dtype=np.float64)
        intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        prm = {"leaf": float(leafsize), "mean_k": int(meanK), "stddev_mul": float(Thresh), "normal_k": int(k),
               "curvature_threshold": float(curvThreshold)}
        pairs, self.stage_rows, self.frame_stats = self.scene.prep_frame(self.boxes, self.depth, intr, prm, return_info=True)
        self.frame_intr = intr
        self.object_mats = [o for o, _ in pairs]
        self.edge_mats = [e for _, e in pairs]
        return pairs

    def RecognizeFrame(self, top: int = 2, min_score: float = 0.0, min_precision: float = 0.0, max_rows: int = 512) -> List[Optional[str]]:
        """Labels without a detector: the object clouds of the last PrepareFrame scored against every detector of
        TrainDetector by their pair-feature keys (``Recognizer``, ppf_recognize_frame).  Sets ``frame_candidates`` -- per
        detection its ``(label, score, precision, recall)`` list, best first, at most ``top`` -- and ``recognize_stats``;
        returns the best label per detection, None where nothing passed ``min_score`` / ``min_precision``: exactly what
        ``MatchFrame(labels)`` takes."""
        if not self.detectors or not all(self.if_trained):
            raise PPFError(_capi.PPF_ERR_NOT_TRAINED, "RecognizeFrame needs the detectors of TrainDetector")
        handles = tuple(d._model for d in self.detectors)
        if self._recognizer is None or self._recognizer[0] != handles:
            self._recognizer = (handles, Recognizer(self.detectors))
        prm = {"top": int(top), "min_score": float(min_score), "min_precision": float(min_precision), "max_rows": int(max_rows)}
        ranked, self.recognize_stats = self._recognizer[1].recognize(self.object_mats, prm, return_stats=True)
        self.frame_candidates = [[(self.id_to_label[int(r["model"])], float(r["score"]), float(r["precision"]), float(r["recall"]))
                                  for r in rows] for rows in ranked]
        return [c[0][0] if c else None for c in self.frame_candidates]

    def MatchFrame(self, labels: Sequence[Optional[str]], relativeSceneSampleStep: float = 0.05,
                   relativeSceneDistance: float = 0.05, one_pass: bool = True) -> List[Optional[Pose3D]]:
        """Matching_S2B (+ ICP of the top 5) of every prepared detection against the model named by labels[i], on the
        resident clouds of PrepareFrame; one pose per detection, None where the label is None, the detection kept no
        points or no pose was found.  By default one ppf_match_frame call matches every detection and refines the top
        poses of all of them in one ICP launch sequence (``timings["match_frame"]``, ``match_frame_stats``);
        ``one_pass=False`` refines detections one after another through Matching_S2B.  Same poses either way."""
        if len(labels) != len(self.object_mats):
            raise PPFError(_capi.PPF_ERR_INVALID, f"{len(labels)} labels for {len(self.object_mats)} prepared detections")
        self.frame_labels = list(labels)
        self.frame_poses = [[] for _ in labels]
        if one_pass:
            return self._match_frame(labels, relativeSceneSampleStep, relativeSceneDistance)
        out: List[Optional[Pose3D]] = []
        for i, (name, obj, edge) in enumerate(zip(labels, self.object_mats, self.edge_mats)):
            if name is None or len(obj) == 0:
                out.append(None)
                continue
            out.append(self.Matching_S2B(name, obj, edge, relativeSceneSampleStep, relativeSceneDistance))
            self.frame_poses[i] = self._last_refined
        return out

    def PoseValidation(self, min_score: float = 0.0, inlier_dist: float = 0.005, depth_tol: float = 0.01, use_depth: bool = True,
                       all_rows: bool = False, normal_cos: Optional[float] = None, *, visibility: str = "facing",
                       render_params=None) -> List[Optional[Pose3D]]:
        """The reference's ``// TODO: Pose Validation`` (CloudProcessing.h:477-479, :530-532): one ppf_verify_frame call scores
        every refined pose the last MatchFrame kept (``frame_poses``) against its detection's object cloud and, with
        ``use_depth`` and a depth image, against ``self.depth``.  Returns per detection its best-scoring pose, or None
        where the detection has no pose or its best score is below ``min_score``.  A float ``normal_cos`` also requires the
        supporting scene row's normal to agree (cos >= normal_cos); ``all_rows`` scores every model row, not only those
        facing the camera.  ``visibility="rendered"`` calls ppf_verify_frame_rendered instead: a model row also has to be
        visible in a surfel z-buffer of its own pose at ``self.depth``'s size (self-occlusion, DESIGN.md §15;
        ``render_params`` as render_frame takes them; not with ``all_rows``).  Sets ``pose_scores``, ``best_index``,
        ``verify_stats`` and ``timings["pose_validation"]``."""
        if visibility not in ("facing", "rendered"):
            raise PPFError(_capi.PPF_ERR_INVALID, f"visibility must be 'facing' or 'rendered', not {visibility!r}")
        dets, poses = [], []
        for name, obj, plist in zip(self.frame_labels, self.object_mats, self.frame_poses):
            if name is None or not plist:
                dets.append(None)
                poses.append([])
                continue
            dets.append((self._model_clouds[self.label_to_id[name]], obj))
            poses.append(plist)
        prm = {"inlier_dist": float(inlier_dist), "depth_tol": float(depth_tol),
               "flags": (_capi.PPF_VERIFY_ALL_ROWS if all_rows else 0) | (_capi.PPF_VERIFY_NORMALS if normal_cos is not None else 0)}
        if normal_cos is not None:
            prm["normal_cos"] = float(normal_cos)
        depth = self.depth if use_depth and self.depth is not None else None
        t0 = time.perf_counter()
        if visibility == "rendered":
            if self.depth is None:
                raise PPFError(_capi.PPF_ERR_INVALID, "PoseValidation(visibility='rendered') renders at the depth image's size")
            self.pose_scores, best, self.verify_stats = verify_frame_rendered(dets, poses, None, depth, self.frame_intr, prm, render_params,
                                                                              image_size=self.depth.shape)
        else:
            self.pose_scores, best, self.verify_stats = verify_frame(dets, poses, None, depth,
                                                                     self.frame_intr if depth is not None else None, prm)
        self.timings["pose_validation"] = time.perf_counter() - t0
        self.best_index = [int(b) for b in best]
        out: List[Optional[Pose3D]] = []
        for i, b in enumerate(self.best_index):
            if b < 0 or float(self.pose_scores[i, b]["score"]) < min_score:
                out.append(None)
            else:
                out.append(self.frame_poses[i][b])
        self.kept_index = [self.best_index[i] if p is not None else -1 for i, p in enumerate(out)]
        return out

    def RenderFrame(self, render_params=None):
        """Depth and instance-label images of the poses the last PoseValidation kept (one ppf_render_frame call at
        ``self.depth``'s size): float32 metres with 0 where no model covers a pixel, and the detection
        index with -1 there.  Sets ``render_stats`` and ``timings["render_frame"]``; returns (depth, label)."""
        if self.depth is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "RenderFrame renders at the depth image's size")
        dets = [None if w < 0 else self._model_clouds[self.label_to_id[self.frame_labels[i]]] for i, w in enumerate(self.kept_index)]
        t0 = time.perf_counter()
        depth, label, self.render_stats = render_frame(dets, self.frame_poses, self.kept_index, self.depth.shape[0], self.depth.shape[1],
                                                       self.frame_intr, render_params, return_stats=True)
        self.timings["render_frame"] = time.perf_counter() - t0
        return depth, label

    def SelectFrame(self, min_score: float = 0.0, max_overlap: float = 0.25, depth_tol: float = 0.01, min_pixels: int = 1,
                    use_scores: bool = False, render_params=None, return_images: bool = False):
        """One consistent set among every refined pose the last MatchFrame kept (one ppf_select_frame call at
        ``self.depth``): duplicates and the same object seen through overlapping boxes are suppressed, a
        second instance inside one box is kept.  ``use_scores`` ranks by the ``score`` of the last PoseValidation instead of
        the explained share.  Returns the selected poses as (detection, k, Pose3D) in selection order; with
        ``return_images`` also the depth and label images (the label is detection * top + k).  Sets ``select_info``,
        ``selected``, ``select_stats`` and ``timings["select_frame"]``."""
        if self.depth is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "SelectFrame needs the depth image")
        if use_scores and self.pose_scores is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "SelectFrame(use_scores=True) needs a PoseValidation first")
        dets = [None if name is None or not plist else self._model_clouds[self.label_to_id[name]]
                for name, plist in zip(self.frame_labels, self.frame_poses)]
        poses = [plist if d is not None else [] for d, plist in zip(dets, self.frame_poses)]
        top = self.pose_scores.shape[1] if use_scores else None
        prm = {"min_score": float(min_score), "max_overlap": float(max_overlap), "depth_tol": float(depth_tol), "min_pixels": int(min_pixels)}
        t0 = time.perf_counter()
        got = select_frame(dets, poses, self.depth, self.frame_intr, prm, render_params, self.pose_scores if use_scores else None, top,
                           return_images=return_images, return_stats=True)
        self.timings["select_frame"] = time.perf_counter() - t0
        self.select_info, self.select_stats = got[0], got[-1]
        top = self.select_info.shape[1] if self.select_info.size else 1
        self.selected = [(int(j) // top, int(j) % top) for j in got[1]]
        out = [(i, k, self.frame_poses[i][k]) for i, k in self.selected]
        return (out, got[2], got[3]) if return_images else out

    def RefineFrame(self, depth=None, selected_only: bool = False, **params) -> List[List[Pose3D]]:
        """The poses held after MatchFrame (``frame_poses``) refined on the depth image itself (one ppf_refine_frame call,
        DESIGN.md §17) and put back into ``frame_poses``, so PoseValidation, SelectFrame and RenderFrame go on with them.
        ``depth``: another frame's image of the same camera (tracking: the poses of the last frame against this frame's
        depth; it becomes ``self.depth``), default ``self.depth`` (polish).  ``selected_only`` refines only the poses the last
        SelectFrame selected and leaves the others as they are.  ``params``: fields of RefineParams.  Sets ``refine_info``,
        ``refine_stats`` and ``timings["refine_frame"]``; returns ``frame_poses``."""
        if depth is not None:
            self.depth = np.ascontiguousarray(depth, dtype=np.float32)
        if self.depth is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "RefineFrame needs the depth image")
        keep = set(self.selected) if selected_only else None
        dets, poses, slots = [], [], []
        for i, (name, plist) in enumerate(zip(self.frame_labels, self.frame_poses)):
            ks = [k for k in range(len(plist)) if keep is None or (i, k) in keep] if name is not None else []
            dets.append(self._model_clouds[self.label_to_id[name]] if ks else None)
            poses.append([plist[k] for k in ks])
            slots.append(ks)
        t0 = time.perf_counter()
        refined, self.refine_info, self.refine_stats = refine_frame(dets, poses, self.depth, self.frame_intr, params or None,
                                                                    return_stats=True)
        self.timings["refine_frame"] = time.perf_counter() - t0
        for i, ks in enumerate(slots):
            for k, p in zip(ks, refined[i]):
                self.frame_poses[i][k] = p
        return self.frame_poses

    def TrackCamera(self, depth, CameraIntr=None, params=None, depth_scale: float = 0.001, z_min: float = 0.0, z_max: float = 0.0):
        """The camera's motion from the processor's depth image (``self.depth``) to ``depth``, the next frame of the same
        camera (one ppf_depth_motion call), applied to every pose of ``frame_poses``: pose <- T pose, so the
        next ``RefineFrame(depth)`` starts from where the camera's motion has carried the objects.  CameraIntr: default
        PrepareFrame's; params: fields of DepthMotionParams.  Sets ``camera_motion`` (T), ``motion_info``, ``motion_stats`` and
        ``timings["track_camera"]``; returns (T, status).  On LOST or STEP the poses stay as they are and T is the identity.
        ``self.depth`` is left alone: RefineFrame(depth) replaces it."""
        intr = self.frame_intr if CameraIntr is None else CameraIntr
        if self.depth is None or intr is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "TrackCamera needs the previous depth image and the camera intrinsics")
        t0 = time.perf_counter()
        T, self.motion_info, self.motion_stats = depth_motion(self.depth, np.ascontiguousarray(depth, dtype=np.float32), intr,
                                                              depth_scale=depth_scale, z_min=z_min, z_max=z_max, params=params,
                                                              return_info=True, return_stats=True)
        self.timings["track_camera"] = time.perf_counter() - t0
        status = int(self.motion_stats["status"])
        if status in (_capi.PPF_MOTION_LOST, _capi.PPF_MOTION_STEP):
            T = np.eye(4)
        else:
            for plist in self.frame_poses:
                for p in plist:
                    _pose_premultiply(p, T)
        self.camera_motion = T
        return T, status

    def FuseVolume(self, depth, CameraIntr=None, volume: Optional[DepthVolume] = None, **fusion):
        """The next frame of a moving camera tracked against, and fused into, a volume the processor owns (``DepthFusion.push``,
        DESIGN.md §30), and the motion applied to every pose of ``frame_poses`` exactly as ``TrackCamera`` does: pose <- T pose.
        CameraIntr: default PrepareFrame's.  The first call makes the ``DepthFusion`` -- on ``volume``, default a
        ``DepthVolume`` of the C defaults, with ``fusion`` (motion_params, raycast_params, depth_scale, z_min, z_max) -- and
        integrates the frame.  Later calls take neither: ``fusion`` keywords are refused once the ``DepthFusion`` exists, and a
        frame of another shape is refused too (the volume holds the first camera's world).  Giving another ``volume`` starts
        afresh on it, with the ``fusion`` keywords given beside it.  Sets
        ``camera_motion`` (T), ``camera_pose`` (the fused world -> camera pose), ``motion_info``, ``motion_stats`` and
        ``timings["fuse_volume"]``; returns (T, status).  On LOST or STEP the poses and the volume stay as they are.
        ``self.depth`` is left alone: RefineFrame(depth) replaces it."""
        intr = self.frame_intr if CameraIntr is None else CameraIntr
        if depth is None or not hasattr(depth, "shape") or len(depth.shape) != 2 or intr is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "FuseVolume needs a 2-D depth image and the camera intrinsics")
        t0 = time.perf_counter()
        f = self._depth_fusion
        afresh = f is None or (volume is not None and volume is not f.volume)
        if not afresh and fusion:
            raise PPFError(_capi.PPF_ERR_INVALID, f"FuseVolume: {', '.join(sorted(fusion))} can only be given with the first frame or a new volume")
        if not afresh and f.shape != tuple(depth.shape):
            raise PPFError(_capi.PPF_ERR_INVALID, f"FuseVolume: the frame is {tuple(depth.shape)}, the volume was started with {f.shape} frames; "
                                                  "give a new volume to start afresh")
        if afresh:
            if volume is None:
                prm = _capi.DepthVolumeParams()
                lib().ppf_default_depth_volume_params(C.byref(prm))
                volume = DepthVolume(tuple(prm.dims), prm.voxel, tuple(prm.origin), prm.trunc, prm.max_weight)
            f = self._depth_fusion = DepthFusion(depth.shape[0], depth.shape[1], intr, volume, **fusion)
        T, status = f.push(depth)
        self.motion_info, self.motion_stats = f.last_info, f.last_stats
        self.timings["fuse_volume"] = time.perf_counter() - t0
        if status not in (_capi.PPF_MOTION_NONE, _capi.PPF_MOTION_LOST, _capi.PPF_MOTION_STEP):
            for plist in self.frame_poses:
                for p in plist:
                    _pose_premultiply(p, T)
        self.camera_motion, self.camera_pose = T, f.pose.copy()
        return T, status

    def MeshVolume(self, path=None, *, keep_largest: Optional[int] = None, min_triangles: Optional[int] = None) -> "VolumeMesh":
        """The triangle mesh of the volume ``FuseVolume`` has filled (``DepthVolume.mesh``), written to ``path``
        as a PLY when a path is given.  A scan is an open surface: give ``LoadMeshModel(path, label, normals="vertex",
        orient=False)`` so that the normals seen through the open back are not flipped.  keep_largest and / or min_triangles
        pass the mesh through ``VolumeMesh.components`` first: only the keep_largest largest pieces, without
        those of fewer than min_triangles triangles; ``mesh_components`` then holds their info.  Both None: the mesh as the
        volume gives it.  Refused before the first ``FuseVolume``."""
        if self._depth_fusion is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "MeshVolume: there is no volume yet; call FuseVolume first")
        t0 = time.perf_counter()
        m = self._depth_fusion.volume.mesh()
        if keep_largest is not None or min_triangles is not None:
            m, self.mesh_components = m.components(min_triangles=1 if min_triangles is None else min_triangles, rank_hi=keep_largest)
        if path is not None:
            m.save_ply(path)
        self.timings["mesh_volume"] = time.perf_counter() - t0
        return m

    def MeshVolumeObjects(self, k: int, min_triangles: int = 1) -> list:
        """The k largest pieces of the volume's mesh that have at least min_triangles triangles, largest first, as
        (vertices, triangles) pairs (``VolumeMesh.split``): a scan of several objects becomes one model each
        through ``LoadMeshModel((vertices, triangles), label, normals="vertex", orient=False)``.  Refused before the first
        ``FuseVolume``."""
        if self._depth_fusion is None:
            raise PPFError(_capi.PPF_ERR_INVALID, "MeshVolumeObjects: there is no volume yet; call FuseVolume first")
        t0 = time.perf_counter()
        pieces = self._depth_fusion.volume.mesh().split(k, min_triangles=min_triangles)
        out = [(p.vertices(), p.triangles()) for p in pieces if p.n_triangles > 0]
        self.timings["mesh_volume_objects"] = time.perf_counter() - t0
        return out

    def _match_frame(self, labels, step, dist, top: int = 5) -> List[Optional[Pose3D]]:
        dets = (FrameDetection * max(len(labels), 1))()
        groups: Dict[bytes, tuple] = {}  # detections whose detectors share match parameters go into one call
        for i, (name, obj, edge) in enumerate(zip(labels, self.object_mats, self.edge_mats)):
            if name is None or len(obj) == 0:
                continue
            idx = self.label_to_id[name]
            if not self.if_trained[idx]:
                raise PPFError(_capi.PPF_ERR_NOT_TRAINED, f"Model [{name}] not trained yet.")
            det = self.detectors[idx]
            if idx not in self._model_clouds:
                self._model_clouds[idx] = DeviceCloud.upload(self.models[idx])
            dets[i].model = det._model.ptr
            dets[i].model_cloud = self._model_clouds[idx]._ptr
            dets[i].scene = obj._ptr
            dets[i].edge = edge._ptr if edge is not None else None
            mp = det._params(step, dist, False)
            groups.setdefault(bytes(mp), (mp, []))[1].append(i)
        prm = IcpParams()
        lib().ppf_default_icp_params(C.byref(prm))
        out: List[Optional[Pose3D]] = [None] * len(labels)
        t0 = time.perf_counter()
        self.match_frame_stats = {}
        for mp, members in groups.values():
            sub = (FrameDetection * len(labels))()
            for i in members:
                sub[i] = dets[i]
            poses = (Pose * (len(labels) * top))()
            n_out = (C.c_int * len(labels))()
            st = MatchFrameStats()
            check(lib().ppf_match_frame(sub, len(labels), C.byref(mp), C.byref(prm), top, poses, n_out, None, C.byref(st)))
            for i in members:
                if n_out[i] > 0:
                    out[i] = Pose3D(poses[i * top])
                    self.frame_poses[i] = [Pose3D(poses[i * top + k]) for k in range(n_out[i])]
            for f, _ in MatchFrameStats._fields_:
                if f != "reserved":
                    self.match_frame_stats[f] = self.match_frame_stats.get(f, 0) + getattr(st, f)
        self.timings["match_frame"] = time.perf_counter() - t0
        return out

    # ---- the PPF half -------------------------------------------------------------------------------------
    def LoadSingleModel(self, model_input: np.ndarray, label: str):
        self.models.append(np.ascontiguousarray(model_input, dtype=np.float32))
        idx = len(self.models) - 1
        self.if_trained.append(False)
        self.label_to_id[label], self.id_to_label[idx] = idx, label
        self.detectors.append(PPF3DDetector(self.relativeSamplingStep, self.relativeDistanceStep))

    def LoadMeshModel(self, mesh_or_path, label: str, spacing: Optional[float] = None, **kw):
        """A model from a triangle mesh: a PLY path (``ply.load_ply_mesh``) or (vertices, triangles), sampled by
        ``DeviceCloud.from_mesh(vertices, triangles, spacing, **kw)`` and stored as LoadSingleModel stores rows.  spacing
        None: half the voxel the trainer will sample with, 0.5 x relativeSamplingStep x the diagonal of the vertices' box.
        Returns the sampling's stats."""
        if isinstance(mesh_or_path, (str, bytes)) or hasattr(mesh_or_path, "__fspath__"):
            from .ply import load_ply_mesh
            vertices, triangles = load_ply_mesh(mesh_or_path)
        else:
            vertices, triangles = mesh_or_path
        vertices = np.ascontiguousarray(vertices, dtype=np.float32)
        if spacing is None:
            if vertices.ndim != 2 or vertices.shape[0] < 1 or vertices.shape[1] < 3:
                raise PPFError(_capi.PPF_ERR_INVALID, "LoadMeshModel: vertices must be (N, 3 | >= 6) float32")
            xyz = vertices[:, :3].astype(np.float64)
            spacing = 0.5 * self.relativeSamplingStep * float(np.linalg.norm(xyz.max(axis=0) - xyz.min(axis=0)))
        kw.pop("return_stats", None)
        cloud, stats = DeviceCloud.from_mesh(vertices, triangles, spacing, return_stats=True, **kw)
        self.LoadSingleModel(cloud.rows(), label)
        return stats

    def TrainDetector(self, relativeSamplingStep_train: float = 0.025, relativeDistanceStep_train: float = 0.5):
        for i, model in enumerate(self.models):
            self.detectors[i] = PPF3DDetector(relativeSamplingStep_train, relativeDistanceStep_train).trainModel(model)
            self.if_trained[i] = True

    def _match(self, name, scene, edge, step, dist) -> Optional[Pose3D]:
        idx = self.label_to_id[name]
        if not self.if_trained[idx]:
            raise PPFError(_capi.PPF_ERR_NOT_TRAINED, f"Model [{name}] not trained yet.")
        det = self.detectors[idx]
        if isinstance(scene, DeviceCloud):
            return self._match_resident(idx, det, scene, edge, step, dist)
        results = det.match(scene, step, dist) if edge is None else det.match_S2B(scene, edge, step, dist)
        if not results:
            return None  # the reference prints "No matching Poses found" and exits (:450-454)
        sub = results[:5]
        ICP(100, 0.005, 2.5, 8).registerModelToScene(self.models[idx], scene, sub)
        return sub[0]

    def _match_resident(self, idx, det, scene: DeviceCloud, edge: Optional[DeviceCloud], step, dist) -> Optional[Pose3D]:
        self._last_refined = []
        mp = det._params(step, dist, False)
        cap = len(scene) + 8
        out = (Pose * cap)()
        n = C.c_int(0)
        t0 = time.perf_counter()
        check(lib().ppf_match_clouds(det._model.ptr, scene._ptr, edge._ptr if edge is not None else None, C.byref(mp), out, cap,
                                     C.byref(n)))
        self.timings["match"] = time.perf_counter() - t0
        if n.value == 0:
            return None
        top = min(5, n.value)
        if idx not in self._model_clouds:
            self._model_clouds[idx] = DeviceCloud.upload(self.models[idx])
        prm = IcpParams()
        lib().ppf_default_icp_params(C.byref(prm))
        t0 = time.perf_counter()
        check(lib().ppf_icp_refine_clouds(self._model_clouds[idx]._ptr, scene._ptr, C.byref(prm), out, top, None))
        self.timings["icp"] = time.perf_counter() - t0
        self._last_refined = [Pose3D(out[k]) for k in range(top)]
        return Pose3D(out[0])

    def Matching(self, name: str, scene: np.ndarray, relativeSceneSampleStep: float = 0.0714,
                 relativeSceneDistance: float = 0.05) -> Optional[Pose3D]:
        return self._match(name, scene, None, relativeSceneSampleStep, relativeSceneDistance)

    def Matching_S2B(self, name: str, scene: np.ndarray, edge: np.ndarray, relativeSceneSampleStep: float = 0.05,
                     relativeSceneDistance: float = 0.05) -> Optional[Pose3D]:
        return self._match(name, scene, edge, relativeSceneSampleStep, relativeSceneDistance)
