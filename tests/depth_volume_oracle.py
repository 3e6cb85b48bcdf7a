"""A numpy restatement of ppf_depth_volume (the comment above ppf_depth_volume_create in include/ppf_hip.h): a
truncated signed distance volume filled from posed depth images, the depth image it gives from any pose and its zero surface
as rows with normals.  Every step is the fp64 arithmetic the kernels do, in the stated order: products are rounded before they
are added (numpy never fuses), the lerps and casts are as written.  z(p) and "kept" are depth_motion_oracle.level0's, which
are ppf_cloud_from_depth's.  The inputs of the tests come from depth_motion_cases (imported as `cases`)."""
import numpy as np

import depth_motion_cases as cases  # noqa: F401  (intrinsics, render, sensor, stream, to_u16 for the tests)
import depth_motion_oracle as MO
from depth_motion_oracle import level0

F32, F64 = np.float32, np.float64
MAX_STEPS = 4096
VOLUME_DEFAULTS = dict(dims=(256, 256, 256), voxel=0.004, origin=(-0.510, -0.510, 0.302), trunc=0.016, max_weight=64)
RAYCAST_DEFAULTS = dict(z_near=0.3, z_far=1.5, ray_step=0.5, min_weight=1)
VOXEL = np.dtype([("d", "<f4"), ("w", "<i4")])


def mat44_mul(A, B):
    """A B as ppf_mat44_mul adds it up: 0 + a0 b0 + a1 b1 + a2 b2 + a3 b3"""
    A, B = np.asarray(A, F64).reshape(4, 4).tolist(), np.asarray(B, F64).reshape(4, 4).tolist()
    out = np.empty((4, 4), F64)
    for i in range(4):
        for j in range(4):
            acc = 0.0
            for k in range(4):
                acc = acc + A[i][k] * B[k][j]
            out[i, j] = acc
    return out


class Volume:
    """d (nz, ny, nx) float32 and w (nz, ny, nx) int32: the records of the device volume, x fastest"""

    def __init__(self, dims, voxel, origin, trunc=None, max_weight=64):
        self.dims = tuple(int(v) for v in dims)
        nx, ny, nz = self.dims
        self.voxel = F32(voxel)
        self.trunc = F32(4) * self.voxel if trunc is None else F32(trunc)
        self.origin = tuple(float(v) for v in origin)
        self.max_weight = int(max_weight)
        self.v64, self.t64 = float(self.voxel), float(self.trunc)
        self.integrations = 0
        self.d = np.ones((nz, ny, nx), F32)
        self.w = np.zeros((nz, ny, nx), np.int32)

    def reset(self):
        self.d[...] = F32(1)
        self.w[...] = 0
        self.integrations = 0

    def records(self):
        """the bytes ppf_depth_volume_read gives, as VOXEL records in linear order"""
        out = np.empty(self.d.size, VOXEL)
        out["d"], out["w"] = self.d.reshape(-1), self.w.reshape(-1)
        return out

    def centres(self):
        """P0 (nx), P1 (ny), P2 (nz): step 1"""
        return [self.origin[a] + np.arange(self.dims[a], dtype=F64) * self.v64 for a in range(3)]


def integrate(vol, img, intr, pose, depth_scale=0.001, z_min=0.0, z_max=0.0):
    """steps 1 to 6 for every voxel at once; returns n_updated"""
    fx, fy, ppx, ppy = (float(v) for v in intr)
    T = np.asarray(pose, F64).reshape(4, 4)
    z = level0(img, depth_scale, z_min, z_max)   # 0 where not kept; a kept z is > 0
    rows, cols = z.shape
    c = vol.centres()
    P0, P1, P2 = c[0][None, None, :], c[1][None, :, None], c[2][:, None, None]
    with np.errstate(all="ignore"):
        p = [((T[r, 0] * P0 + T[r, 1] * P1) + T[r, 2] * P2) + T[r, 3] for r in range(3)]
        ok = p[2] > 0
        uf = np.floor((p[0] * fx / p[2] + ppx) + 0.5)
        vf = np.floor((p[1] * fy / p[2] + ppy) + 0.5)
        ok &= (uf >= 0) & (uf < cols) & (vf >= 0) & (vf < rows)
        ui, vi = np.where(ok, uf, 0).astype(np.int64), np.where(ok, vf, 0).astype(np.int64)
        zp = z[vi, ui]
        ok &= zp > 0
        sdf = zp.astype(F64) - p[2]
        ok &= ~(sdf < -vol.t64)
        dn = sdf / vol.t64
        dn = np.where(dn > 1.0, 1.0, dn)
        new = ((vol.d.astype(F64) * vol.w.astype(F64) + dn) / (vol.w + 1).astype(F64)).astype(F32)
    vol.d = np.where(ok, new, vol.d)
    vol.w = np.where(ok, np.minimum(vol.w + 1, vol.max_weight), vol.w).astype(np.int32)
    vol.integrations += 1
    return int(ok.sum())


def near(vol, P, min_weight):
    """near(P) for arrays P[0..2]: (exists, (double)d)"""
    nx, ny, nz = vol.dims
    with np.errstate(all="ignore"):
        idx = [np.floor((P[a] - vol.origin[a]) / vol.v64 + 0.5) for a in range(3)]
        inside = (idx[0] >= 0) & (idx[0] < nx) & (idx[1] >= 0) & (idx[1] < ny) & (idx[2] >= 0) & (idx[2] < nz)
        i, j, k = (np.where(inside, v, 0).astype(np.int64) for v in idx)
    ok = inside & (vol.w[k, j, i] >= min_weight)
    return ok, vol.d[k, j, i].astype(F64)


def tri(vol, P, min_weight):
    """tri(P) for arrays P[0..2]: (exists, value): four lerps along x, two along y, one along z"""
    nx, ny, nz = vol.dims
    with np.errstate(all="ignore"):
        g = [(P[a] - vol.origin[a]) / vol.v64 for a in range(3)]
        b = [np.floor(v) for v in g]
        inside = (b[0] >= 0) & (b[0] + 1.0 < nx) & (b[1] >= 0) & (b[1] + 1.0 < ny) & (b[2] >= 0) & (b[2] + 1.0 < nz)
        f = [g[a] - b[a] for a in range(3)]
        i, j, k = (np.where(inside, v, 0).astype(np.int64) for v in b)
        i1, j1, k1 = np.minimum(i + 1, nx - 1), np.minimum(j + 1, ny - 1), np.minimum(k + 1, nz - 1)
        ok = inside.copy()
        c = {}
        for dz, kk in ((0, k), (1, k1)):
            for dy, jj in ((0, j), (1, j1)):
                for dx, ii in ((0, i), (1, i1)):
                    ok &= vol.w[kk, jj, ii] >= min_weight
                    c[dx, dy, dz] = vol.d[kk, jj, ii].astype(F64)
        x00 = c[0, 0, 0] + f[0] * (c[1, 0, 0] - c[0, 0, 0])
        x10 = c[0, 1, 0] + f[0] * (c[1, 1, 0] - c[0, 1, 0])
        x01 = c[0, 0, 1] + f[0] * (c[1, 0, 1] - c[0, 0, 1])
        x11 = c[0, 1, 1] + f[0] * (c[1, 1, 1] - c[0, 1, 1])
        y0 = x00 + f[1] * (x10 - x00)
        y1 = x01 + f[1] * (x11 - x01)
        return ok, y0 + f[2] * (y1 - y0)


def ray_steps(vol, z_near, z_far, ray_step):
    """(step, K)"""
    step = float(F32(ray_step)) * vol.t64
    return step, int(np.ceil((float(F32(z_far)) - float(F32(z_near))) / step))


def rays(shape, intr, pose):
    """(c (3), dw: three (rows, cols) arrays, R)"""
    fx, fy, ppx, ppy = (float(v) for v in intr)
    T = np.asarray(pose, F64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    c = [-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2]) for a in range(3)]
    u = np.arange(shape[1], dtype=F64)[None, :] + np.zeros(shape, F64)
    v = np.arange(shape[0], dtype=F64)[:, None] + np.zeros(shape, F64)
    dc = [(u - ppx) / fx, (v - ppy) / fy, np.ones(shape, F64)]
    dw = [(R[0, a] * dc[0] + R[1, a] * dc[1]) + R[2, a] * dc[2] for a in range(3)]
    return c, dw, R


def walk(vol, c, dw, z_near, step, K, min_weight):
    """the march for every pixel at once: (hit, k of the back sample, f of sample k - 1, f of sample k)"""
    shape = dw[0].shape
    done = np.zeros(shape, bool)
    kb = np.full(shape, -1, np.int64)
    prev_front = np.zeros(shape, bool)
    fp, fk = np.zeros(shape, F64), np.zeros(shape, F64)
    zn = float(F32(z_near))
    for k in range(K):
        if done.all():
            break
        s = zn + float(k) * step
        some, d = near(vol, [c[a] + s * dw[a] for a in range(3)], min_weight)
        back = some & ~(d > 0) & ~done
        kb = np.where(back, k, kb)
        fk = np.where(back, d, fk)
        done |= back
        prev_front = np.where(done, prev_front, some)
        fp = np.where(done, fp, d)
    return (kb >= 1) & prev_front, kb, fp, fk


def raycast(vol, shape, intr, pose, z_near=0.3, z_far=1.5, ray_step=0.5, min_weight=1, normals=False):
    """(depth (rows, cols) float32, normals (rows, cols, 3) float32 or None, stats)"""
    step, K = ray_steps(vol, z_near, z_far, ray_step)
    assert 1 <= K <= MAX_STEPS
    c, dw, R = rays(shape, intr, pose)
    hit, kb, fp, fk = walk(vol, c, dw, z_near, step, K, min_weight)
    zn = float(F32(z_near))
    with np.errstate(all="ignore"):
        s0 = zn + (kb - 1).astype(F64) * step
        s1 = zn + kb.astype(F64) * step
        h0, a0 = tri(vol, [c[a] + s0 * dw[a] for a in range(3)], min_weight)
        h1, a1 = tri(vol, [c[a] + s1 * dw[a] for a in range(3)], min_weight)
        use = hit & h0 & h1 & (a0 > 0) & (0 >= a1)
        f0, f1 = np.where(use, a0, fp), np.where(use, a1, fk)
        ss = s0 + step * f0 / (f0 - f1)
        depth = np.where(hit, ss, 0.0).astype(F32)
    out_n = None
    if normals:
        with np.errstate(all="ignore"):
            X = [c[a] + ss * dw[a] for a in range(3)]
            ok, g = hit.copy(), []
            for a in range(3):
                hi = tri(vol, [X[b] + vol.v64 if b == a else X[b] for b in range(3)], min_weight)
                lo = tri(vol, [X[b] - vol.v64 if b == a else X[b] for b in range(3)], min_weight)
                ok &= hi[0] & lo[0]
                g.append(hi[1] - lo[1])
            ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            ok &= ln > 0
            nw = [g[a] / ln for a in range(3)]
            out_n = np.stack([np.where(ok, (R[r, 0] * nw[0] + R[r, 1] * nw[1]) + R[r, 2] * nw[2], 0.0) for r in range(3)], axis=-1).astype(F32)
    stats = dict(n_hits=int(hit.sum()), n_interpolated=int(use.sum()), n_launches=1, n_host_syncs=1)
    return depth, out_n, stats


def gradients(vol, min_weight):
    """(defined (nz, ny, nx), g: three (nz, ny, nx) float64): the central differences at every lattice voxel"""
    d, seen = vol.d.astype(F64), vol.w >= min_weight
    ok = np.zeros(vol.d.shape, bool)
    g = [np.zeros(vol.d.shape, F64) for _ in range(3)]
    if min(vol.d.shape) >= 3:
        m = (slice(1, -1),) * 3
        ok[m] = True
        for a, ax in enumerate((2, 1, 0)):   # x is the last array axis
            hi = tuple(slice(2, None) if q == ax else slice(1, -1) for q in range(3))
            lo = tuple(slice(0, -2) if q == ax else slice(1, -1) for q in range(3))
            ok[m] &= seen[hi] & seen[lo]
            g[a][m] = d[hi] - d[lo]
    return ok, g


def extract(vol, min_weight=1):
    """(rows (n, 6) float32 in (linear voxel index, axis) order, stats)"""
    d, seen = vol.d.astype(F64), vol.w >= min_weight
    gok, g = gradients(vol, min_weight)
    c = vol.centres()
    P = np.meshgrid(c[2], c[1], c[0], indexing="ij")[::-1]   # P[0] = x of every voxel, ...
    shape = vol.d.shape
    flag = np.zeros(shape + (3,), bool)
    cross = np.zeros(shape + (3,), bool)
    rows = np.zeros(shape + (3, 6), F32)
    for a, ax in enumerate((2, 1, 0)):
        if shape[ax] < 2:
            continue
        me = tuple(slice(0, -1) if q == ax else slice(None) for q in range(3))
        nb = tuple(slice(1, None) if q == ax else slice(None) for q in range(3))
        d0, d1 = d[me], d[nb]
        with np.errstate(all="ignore"):
            x = seen[me] & seen[nb] & (np.abs(d0) < 1) & (np.abs(d1) < 1) & ((d0 > 0) != (d1 > 0))
            t = d0 / (d0 - d1)
            gg = [g[b][me] + t * (g[b][nb] - g[b][me]) for b in range(3)]
            ln = np.sqrt((gg[0] * gg[0] + gg[1] * gg[1]) + gg[2] * gg[2])
            ok = x & gok[me] & gok[nb] & (ln > 0)
            cross[me + (a,)] = x
            flag[me + (a,)] = ok
            for b in range(3):
                rows[me + (a, b)] = (P[b][me] + t * vol.v64 if b == a else P[b][me]).astype(F32)
                rows[me + (a, 3 + b)] = (gg[b] / ln).astype(F32)
    out = rows.reshape(-1, 6)[flag.reshape(-1)]
    stats = dict(n_crossings=int(cross.sum()), n_rows=int(flag.sum()), n_launches=7, n_host_syncs=2)
    return np.ascontiguousarray(out), stats


def metres(img, depth_scale=0.001):
    """a uint16 image as float32 metres, z = (float)((double)d * depth_scale); a float32 image as it is"""
    img = np.asarray(img)
    return (img.astype(F64) * F64(depth_scale)).astype(F32) if img.dtype == np.uint16 else img.astype(F32)


class Fusion:
    """DepthFusion by the oracles: frame-to-model tracking on a Volume"""

    def __init__(self, shape, intr, vol, motion_params=None, raycast_params=None, depth_scale=0.001, z_min=0.0, z_max=0.0):
        self.shape, self.intr, self.vol = tuple(shape), tuple(float(v) for v in intr), vol
        self.mp, self.rp = motion_params, dict(RAYCAST_DEFAULTS, **(raycast_params or {}))
        self.kw = dict(depth_scale=depth_scale, z_min=z_min, z_max=z_max)
        self.pose, self.frames, self.model_depth = np.eye(4), 0, None

    def push(self, depth):
        if self.frames == 0:
            integrate(self.vol, depth, self.intr, self.pose, **self.kw)
            self.frames = 1
            return np.eye(4), MO.NONE
        self.model_depth = raycast(self.vol, self.shape, self.intr, self.pose, **self.rp)[0]
        cur = metres(depth, self.kw["depth_scale"])   # one format for both images: float32 metres
        T, _, stats = MO.motion(self.model_depth, cur, self.intr, self.mp, z_min=self.kw["z_min"], z_max=self.kw["z_max"])
        self.frames += 1
        if stats["status"] in (MO.LOST, MO.STEP):
            return np.eye(4), stats["status"]
        self.pose = mat44_mul(T, self.pose)
        integrate(self.vol, depth, self.intr, self.pose, **self.kw)
        return T, stats["status"]
