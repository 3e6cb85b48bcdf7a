"""Seeded inputs for ppf_depth_motion that the CPU tests of tests/depth_motion_oracle.py (tests/test_depth_motion_oracle.py) and
the device tests (tests/test_gpu_depth_motion.py) share: an analytic scene of three planes and three spheres 0.5 to 1.0 m from
the camera, ray-cast exactly (float64 z, rounded to float32 once), seeded camera motions, sensor noise and dropped pixels.

A frame pair is (prev, cur, T_true): prev is the scene seen from the camera at the origin, cur the scene seen after the
camera's motion, and T_true takes a static point's coordinates in the previous camera frame to the current one."""
import functools

import numpy as np

import refine_oracle as R

F32, F64 = np.float32, np.float64
ROWS, COLS = 120, 160
FOCAL = 150.0

# planes n . x = d (n towards the camera's half space does not matter: the nearest positive hit wins) and spheres (centre, radius),
# in the first camera's frame: a back wall, a floor and a side wall that meet in a corner, three spheres in front of them
PLANES = [((0.10, 0.05, 1.0), 1.00), ((0.0, 1.0, 0.8), 1.00), ((1.0, 0.0, 0.8), 1.10)]
SPHERES = [((-0.12, -0.05, 0.72), 0.09), ((0.10, 0.08, 0.62), 0.07), ((0.02, -0.16, 0.80), 0.08)]


def intrinsics(rows=ROWS, cols=COLS, focal=None):
    """(fx, fy, ppx, ppy) of a rows x cols camera with the field of view of the 120 x 160, f = 150 one"""
    f = FOCAL * cols / COLS if focal is None else focal
    return (f, f, (cols - 1) / 2.0, (rows - 1) / 2.0)


def render(T, rows=ROWS, cols=COLS, intr=None):
    """the exact depth image (float64 z, 0 where no surface is hit) of the scene from the camera whose frame T (4 x 4: first
    camera's frame -> this camera's) defines"""
    fx, fy, ppx, ppy = intrinsics(rows, cols) if intr is None else intr
    T = np.asarray(T, dtype=F64).reshape(4, 4)
    Rm, t = T[:3, :3], T[:3, 3]
    u, v = np.meshgrid(np.arange(cols, dtype=F64), np.arange(rows, dtype=F64))
    d = np.stack([(u - ppx) / fx, (v - ppy) / fy, np.ones_like(u)], axis=-1)   # z = 1: the ray parameter is z
    z = np.full((rows, cols), np.inf)
    with np.errstate(all="ignore"):
        for n, off in PLANES:
            n = np.asarray(n, F64)
            off = off / np.linalg.norm(n)
            n = n / np.linalg.norm(n)
            n2 = Rm @ n
            off2 = off + n2 @ t
            s = off2 / (d @ n2)
            z = np.where((s > 0) & (s < z), s, z)
        for c, rad in SPHERES:
            c2 = Rm @ np.asarray(c, F64) + t
            a = (d * d).sum(-1)
            b = d @ c2
            disc = b * b - a * (c2 @ c2 - rad * rad)
            s = (b - np.sqrt(disc)) / a
            z = np.where((disc >= 0) & (s > 0) & (s < z), s, z)
    return np.where(np.isfinite(z), z, 0.0)


def true_motion(seed, mm, deg):
    """a camera motion of mm millimetres and deg degrees, both in the random directions of `seed`"""
    t, r = R.random_offset(np.random.default_rng(seed), mm, deg)
    T = np.eye(4)
    T[:3, :3] = R.rot_vec(r)
    T[:3, 3] = t
    return T


def sensor(z, seed, noise=0.002, drop=0.05):
    """z with Gaussian noise of sigma noise * z^2 and one pixel in 1 / drop set to 0, as float32"""
    rng = np.random.default_rng(seed)
    out = z + rng.normal(size=z.shape) * noise * z * z
    out[rng.random(z.shape) < drop] = 0.0
    return np.where(z > 0, out, 0.0).astype(F32)


@functools.lru_cache(maxsize=None)
def pair(seed, mm, deg, rows=ROWS, cols=COLS, noise=0.002, drop=0.05):
    """(prev, cur, T_true): float32 images of the scene before and after the motion of `seed`; noise 0 and drop 0: exact"""
    T = true_motion(seed, mm, deg)
    prev, cur = render(np.eye(4), rows, cols), render(T, rows, cols)
    if noise or drop:
        prev, cur = sensor(prev, 2 * seed + 1000, noise, drop), sensor(cur, 2 * seed + 1001, noise, drop)
    else:
        prev, cur = prev.astype(F32), cur.astype(F32)
    prev.setflags(write=False)
    cur.setflags(write=False)
    return prev, cur, T


ACCURACY_SEEDS = tuple(range(8))   # the 8 draws of 30 mm / 3 degrees at 120 x 160, three levels


def spoiled(img, seed):
    """a copy of a float32 image with holes, NaN, +-inf and negative pixels sprinkled in"""
    rng = np.random.default_rng(seed)
    out = np.array(img, dtype=F32)
    flat = out.reshape(-1)
    for value in (0.0, np.nan, np.inf, -np.inf, -0.5):
        flat[rng.choice(flat.size, size=max(1, flat.size // 97), replace=False)] = value
    return out


def to_u16(img, depth_scale=0.001):
    """the image in sensor units of depth_scale metres"""
    return np.clip(np.rint(np.asarray(img, F64) / depth_scale), 0, 65535).astype(np.uint16)


def pitched(img, pad, offset=0):
    """the image as a view with `pad` extra elements per row, starting `offset` elements into its buffer"""
    rows, cols = img.shape
    buf = np.zeros(offset + rows * (cols + pad), dtype=img.dtype)
    view = buf[offset:].reshape(rows, cols + pad)[:, :cols]
    view[...] = img
    return view


def stream(n_frames, seed, mm, deg, rows=ROWS, cols=COLS):
    """n_frames noisy images of a camera that moves by (mm, deg) in a new seeded direction between frames, and the true camera
    poses (first camera's frame -> frame i's)"""
    poses = [np.eye(4)]
    for i in range(1, n_frames):
        poses.append(true_motion(seed + i, mm, deg) @ poses[-1])
    return [sensor(render(P, rows, cols), 77 * seed + i) for i, P in enumerate(poses)], poses
