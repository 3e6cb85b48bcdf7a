"""Seeded inputs for ppf_depth_volume that the CPU tests of tests/depth_volume_oracle.py (tests/test_depth_volume_oracle.py) and
the device tests (tests/test_gpu_depth_volume.py) share.  The analytic scene, its camera, the sensor model and the streams are
depth_motion_cases'; added here are a sphere of 0.1 m at 0.7 m seen from four sides, the volumes both are fused into, and small
images of the scene for the small volumes of the device tests."""
import functools

import numpy as np

import depth_motion_cases as cases
import refine_oracle as R

F32, F64 = np.float32, np.float64
SHAPE = (cases.ROWS, cases.COLS)
SPHERE_C, SPHERE_R = np.array([0.0, 0.0, 0.7]), 0.1
SCENE_VOLUME = dict(dims=(96, 96, 96), voxel=0.010, origin=(-0.475, -0.475, 0.355), trunc=0.04)     # the whole analytic scene
SPHERE_VOLUME = dict(dims=(64, 64, 64), voxel=0.005, origin=(-0.1575, -0.1575, 0.5425), trunc=0.02)  # a cube around the sphere
SCENE_RAYCAST = dict(z_near=0.3, z_far=1.4)
SPHERE_RAYCAST = dict(z_near=0.4, z_far=1.0)


def render_sphere(T, shape=SHAPE, intr=None):
    """the exact float32 depth image of the sphere alone from the camera of T (world -> camera), 0 beside it"""
    fx, fy, ppx, ppy = cases.intrinsics(*shape) if intr is None else intr
    T = np.asarray(T, F64).reshape(4, 4)
    c2 = T[:3, :3] @ SPHERE_C + T[:3, 3]
    u, v = np.meshgrid(np.arange(shape[1], dtype=F64), np.arange(shape[0], dtype=F64))
    d = np.stack([(u - ppx) / fx, (v - ppy) / fy, np.ones_like(u)], -1)
    a, b = (d * d).sum(-1), d @ c2
    disc = b * b - a * (c2 @ c2 - SPHERE_R * SPHERE_R)
    with np.errstate(all="ignore"):
        s = (b - np.sqrt(disc)) / a
    return np.where(disc >= 0, s, 0.0).astype(F32)


def look(angle_y, angle_x):
    """the pose of a camera turned about the sphere's centre, which stays 0.7 m ahead on the optical axis"""
    Rm = R.rot_vec(np.array([angle_x, angle_y, 0.0]))
    T = np.eye(4)
    T[:3, :3] = Rm
    T[:3, 3] = SPHERE_C - Rm @ SPHERE_C
    return T


SPHERE_VIEWS = (look(0.0, 0.0), look(0.5, 0.0), look(-0.5, 0.1), look(0.1, 0.5))


@functools.lru_cache(maxsize=None)
def sphere_frames():
    out = [render_sphere(T) for T in SPHERE_VIEWS]
    for f in out:
        f.setflags(write=False)
    return out


SCAN_OBJECTS = (((-0.055, 0.0, 0.70), (0.06, 0.06, 0.06)), ((0.065, 0.01, 0.70), (0.04, 0.07, 0.05)))   # (centre, semi-axes)


def render_scan(T, shape=SHAPE, intr=None):
    """the exact float32 depth image of a sphere and an ellipsoid side by side inside SPHERE_VOLUME, 0 beside them"""
    fx, fy, ppx, ppy = cases.intrinsics(*shape) if intr is None else intr
    T = np.asarray(T, F64).reshape(4, 4)
    Rm, t = T[:3, :3], T[:3, 3]
    u, v = np.meshgrid(np.arange(shape[1], dtype=F64), np.arange(shape[0], dtype=F64))
    d = np.stack([(u - ppx) / fx, (v - ppy) / fy, np.ones_like(u)], -1) @ Rm   # the ray in world coordinates, per unit of z
    o = -Rm.T @ t
    z = np.full(shape, np.inf)
    with np.errstate(all="ignore"):
        for c, axes in SCAN_OBJECTS:
            axes = np.asarray(axes, F64)
            oo, dd = (o - np.asarray(c, F64)) / axes, d / axes
            a, b = (dd * dd).sum(-1), dd @ oo
            disc = b * b - a * (oo @ oo - 1.0)
            s = (-b - np.sqrt(disc)) / a
            z = np.where((disc >= 0) & (s > 0) & (s < z), s, z)
    return np.where(np.isfinite(z), z, 0.0).astype(F32)


def compare(depth, truth):
    """(rms, worst, median of |depth - truth| where both have a value; the share of truth's pixels that depth has too)"""
    both = (depth > 0) & (truth > 0)
    err = np.abs(depth[both].astype(F64) - truth[both].astype(F64))
    return float(np.sqrt((err * err).mean())), float(err.max()), float(np.median(err)), float(both.sum()) / float((truth > 0).sum())


def small_frame(rows, cols, seed=0, T=None):
    """a noisy rows x cols float32 image of the analytic scene from the camera of T (default: the first camera)"""
    z = cases.render(np.eye(4) if T is None else T, rows, cols)
    return cases.sensor(z, 500 + seed)


def box_volume(dims, voxel=0.01, z0=0.6, max_weight=64):
    """parameters of a volume of `dims` voxels of `voxel` metres, about centred on the optical axis, from z0 on; trunc 2.5 voxels"""
    voxel = float(F32(voxel))
    origin = (-voxel * (dims[0] - 1) / 2.0 + 0.003, -voxel * (dims[1] - 1) / 2.0 - 0.002, z0)
    return dict(dims=tuple(dims), voxel=voxel, origin=origin, trunc=float(F32(2.5) * F32(voxel)), max_weight=max_weight)


def box_frame(vp, rows, cols, seed, dtype=F32):
    """(image, intr) for the volume vp seen from the world's origin: a smooth noisy surface through the volume's middle that
    leans across its depth, through a camera whose image is a little narrower than the volume, so some voxels fall outside"""
    dims, voxel = vp["dims"], vp["voxel"]
    ext = [max(d - 1, 1) * voxel for d in dims]
    zc = vp["origin"][2] + (dims[2] - 1) * voxel / 2.0
    f = (cols / 2.0) * zc / (0.4 * max(ext[0], ext[1]) + 0.5 * voxel)
    intr = (f, f * 1.05, (cols - 1) / 2.0 + 0.25, (rows - 1) / 2.0 - 0.4)
    rng = np.random.default_rng(seed)
    xn = np.linspace(-1, 1, cols)[None, :] + np.zeros((rows, cols))
    yn = np.linspace(-1, 1, rows)[:, None] + np.zeros((rows, cols))
    z = zc + 0.35 * ext[2] * (xn + 0.5 * yn) + rng.normal(size=(rows, cols)) * 0.1 * voxel + 0.002 * (seed % 5)
    img = z.astype(F32)
    return (cases.to_u16(img, 0.001) if dtype == np.uint16 else img), intr


def box_pose(vp, kind, seed=0):
    """identity; a small seeded motion; the camera moved forward so that the volume's near half lies behind it; or moved
    sideways so that much of the volume leaves the image"""
    T = np.eye(4) if kind == "identity" else cases.true_motion(seed, 8.0, 2.0)
    if kind == "behind":
        T[2, 3] -= vp["origin"][2] + (vp["dims"][2] - 1) * vp["voxel"] / 2.0 - 0.3 * vp["voxel"]
    if kind == "aside":
        T[0, 3] += 0.45 * max(vp["dims"][0] - 1, 1) * vp["voxel"]
    return T


def small_volume(dims, span=0.5, z0=0.45):
    """parameters of a volume of `dims` voxels that covers about span metres across the optical axis, from z0 on: the voxel is
    what the largest dimension needs, trunc four voxels"""
    voxel = float(F32(span / max(max(dims), 2)))
    origin = (-voxel * (dims[0] - 1) / 2.0 + 0.003, -voxel * (dims[1] - 1) / 2.0 - 0.002, z0)
    return dict(dims=tuple(dims), voxel=voxel, origin=origin, trunc=float(F32(4) * F32(voxel)))
