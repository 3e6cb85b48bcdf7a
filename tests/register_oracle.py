"""numpy restatement of the depth registration specification (include/ppf_camera_math.h): the camera model
operation for operation in fp64, the vertices, quads and triangles of ppf_depth_register, and the fixture cameras of its
tests.  Everything the device computes must equal this byte for byte; tests/test_register_oracle.py holds this file to
properties that do not depend on it (an analytic plane, a box in front of it)."""
import numpy as np

NEWTON_ITERS = 7          # PPF_CAMERA_NEWTON_ITERS
MAX_RESIDUAL = 1e-18      # PPF_CAMERA_MAX_RESIDUAL
MAX_QUAD_PX = 16          # PPF_REGISTER_MAX_QUAD_PX
EMPTY = np.uint32(0xFFFFFFFF)


class Cam:
    FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6", "max_r")

    def __init__(self, fx, fy, cx, cy, k=(0.0,) * 6, p=(0.0, 0.0), max_r=0.0):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.k1, self.k2, self.k3, self.k4, self.k5, self.k6 = [float(v) for v in k]
        self.p1, self.p2 = [float(v) for v in p]
        self.max_r = float(max_r)

    def values(self):
        return [getattr(self, f) for f in self.FIELDS]

    def scaled(self, s, cx, cy):
        """the same lens on an image s times as large"""
        c = Cam(self.fx * s, self.fy * s, cx, cy, max_r=self.max_r)
        for f in self.FIELDS[4:12]:
            setattr(c, f, getattr(self, f))
        return c


# Kinect-like coefficients on small images: (camera, rows, cols)
DEPTH_CAM = (Cam(50.4, 50.4, 31.6, 27.3, (5.0, 3.2, 0.17, 5.3, 4.9, 0.9), (1e-4, -5e-5)), 48, 64)
COLOR_CAM = (Cam(57.0, 57.0, 59.5, 44.5, (0.45, -2.5, 1.5, 0.33, -2.3, 1.4), (5e-4, -3e-4)), 90, 120)


def extrinsics(deg=6.0, t=(-0.032, -0.002, 0.004)):
    """a rotation about x and a translation, depth frame -> colour frame"""
    a = np.deg2rad(deg)
    R = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    return R, np.asarray(t, np.float64)


def over_max_r(c, x, y):
    if c.max_r == 0.0:
        return np.zeros(np.shape(x), bool)
    return x * x + y * y > c.max_r * c.max_r


def distort(c, x, y, jac=False):
    """ppf_cam_distort: (xd, yd, ok[, J00, J01, J10, J11])"""
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    a = 1.0 + c.k1 * r2 + c.k2 * r4 + c.k3 * r6
    b = 1.0 + c.k4 * r2 + c.k5 * r4 + c.k6 * r6
    d = a / b
    xd = x * d + 2.0 * c.p1 * x * y + c.p2 * (r2 + 2.0 * x * x)
    yd = y * d + c.p1 * (r2 + 2.0 * y * y) + 2.0 * c.p2 * x * y
    ok = (b != 0.0) & np.isfinite(d)
    if not jac:
        return xd, yd, ok
    a1 = c.k1 + 2.0 * c.k2 * r2 + 3.0 * c.k3 * r4
    b1 = c.k4 + 2.0 * c.k5 * r2 + 3.0 * c.k6 * r4
    d1 = (a1 * b - a * b1) / (b * b)
    dx = d1 * (2.0 * x)
    dy = d1 * (2.0 * y)
    j00 = d + x * dx + 2.0 * c.p1 * y + 6.0 * c.p2 * x
    j01 = x * dy + 2.0 * c.p1 * x + 2.0 * c.p2 * y
    j10 = y * dx + 2.0 * c.p1 * x + 2.0 * c.p2 * y
    j11 = d + y * dy + 6.0 * c.p1 * y + 2.0 * c.p2 * x
    return xd, yd, ok, j00, j01, j10, j11


def project(c, x, y):
    """ppf_cam_project on arrays: (u, v, valid), NaN where invalid"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        xd, yd, ok = distort(c, x, y)
        u = c.fx * xd + c.cx
        v = c.fy * yd + c.cy
        ok = ok & np.isfinite(u) & np.isfinite(v) & ~over_max_r(c, x, y)
    return np.where(ok, u, np.nan), np.where(ok, v, np.nan), ok


def unproject(c, u, v, iters=NEWTON_ITERS, check=True):
    """ppf_cam_unproject on arrays: (x, y, valid), NaN where invalid; check=False: the raw iterate (for the convergence table)"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        xd = (u - c.cx) / c.fx
        yd = (v - c.cy) / c.fy
        x, y = xd, yd
        ok = np.ones(x.shape, bool)
        for _ in range(iters):
            fx, fy, _, j00, j01, j10, j11 = distort(c, x, y, jac=True)
            e0 = fx - xd
            e1 = fy - yd
            det = j00 * j11 - j01 * j10
            ok = ok & ~(det == 0.0)
            x, y = x - (j11 * e0 - j01 * e1) / det, y - (j00 * e1 - j10 * e0) / det
        if not check:
            return x, y, ok
        fx, fy, bok = distort(c, x, y)
        e0 = fx - xd
        e1 = fy - yd
        res = e0 * e0 + e1 * e1
        ok = ok & bok & np.isfinite(x) & np.isfinite(y) & np.isfinite(res) & (res <= MAX_RESIDUAL) & ~over_max_r(c, x, y)
    return np.where(ok, x, np.nan), np.where(ok, y, np.nan), ok


def pixel_grid(rows, cols):
    vv, uu = np.mgrid[0:rows, 0:cols]
    return uu.astype(np.float64), vv.astype(np.float64)


def rays(cam, rows, cols):
    """ppf_depth_map_rays: [rows][cols][2], NaN NaN = invalid"""
    uu, vv = pixel_grid(rows, cols)
    x, y, _ = unproject(cam, uu, vv)
    return np.stack([x, y], axis=-1)


def map_boxes(cfrom, cto, to_rows, to_cols, boxes):
    """ppf_camera_map_boxes"""
    out = np.zeros((len(boxes), 4), np.int32)
    for i, (bx, by, bw, bh) in enumerate(np.asarray(boxes, np.int64).reshape(-1, 4)):
        xs = [float(bx), float(bx) + float(bw) / 2.0, float(bx) + float(bw)]
        ys = [float(by), float(by) + float(bh) / 2.0, float(by) + float(bh)]
        pts = [(xs[ix], ys[iy]) for iy in range(3) for ix in range(3) if not (ix == 1 and iy == 1)]
        x, y, ok1 = unproject(cfrom, np.array([p[0] for p in pts]), np.array([p[1] for p in pts]))
        u, v, ok2 = project(cto, x, y)
        ok = ok1 & ok2
        if not ok.any():
            continue
        u0, u1 = np.floor(u[ok].min()), np.ceil(u[ok].max())
        v0, v1 = np.floor(v[ok].min()), np.ceil(v[ok].max())
        u0, u1 = np.clip([u0, u1], 0.0, float(to_cols))
        v0, v1 = np.clip([v0, v1], 0.0, float(to_rows))
        if u1 - u0 <= 0.0 or v1 - v0 <= 0.0:
            continue
        out[i] = [int(u0), int(v0), int(u1 - u0), int(v1 - v0)]
    return out


def kept_depth(depth, depth_scale=0.001, z_min=0.0, z_max=0.0):
    """(z float32, keep): the kept-pixel rule of ppf_cloud_from_depth"""
    z = depth if depth.dtype == np.float32 else (depth.astype(np.float64) * depth_scale).astype(np.float32)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(z) & (z > 0) & (z >= np.float32(z_min)) & ((np.float32(z_max) == 0) | (z <= np.float32(z_max)))
    return z, keep


def _draw(zbuf, cols, rows, tri, A, B, Cv):
    """the triangles tri (indices) with vertices A, B, C = (u, v, z) arrays; returns (the oversize flags, the largest box side drawn)"""
    (ax, ay, az), (bx, by, bz), (cx, cy, cz) = [[w[tri] for w in V] for V in (A, B, Cv)]
    x0 = np.ceil(np.minimum(np.minimum(ax, bx), cx))
    x1 = np.floor(np.maximum(np.maximum(ax, bx), cx))
    y0 = np.ceil(np.minimum(np.minimum(ay, by), cy))
    y1 = np.floor(np.maximum(np.maximum(ay, by), cy))
    x0, y0 = np.maximum(x0, 0.0), np.maximum(y0, 0.0)               # clamped as doubles, before the conversion to int
    x1, y1 = np.minimum(x1, float(cols - 1)), np.minimum(y1, float(rows - 1))
    empty = (x1 < x0) | (y1 < y0)
    over = ~empty & ((x1 - x0 >= float(MAX_QUAD_PX)) | (y1 - y0 >= float(MAX_QUAD_PX)))
    with np.errstate(all="ignore"):
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        go = ~empty & ~over & (area != 0.0)
        i0, j0 = np.where(go, x0, 0).astype(np.int64), np.where(go, y0, 0).astype(np.int64)
        i1, j1 = np.where(go, x1, -1).astype(np.int64), np.where(go, y1, -1).astype(np.int64)
        W = int((i1 - i0).max()) + 1 if go.any() else 0
        H = int((j1 - j0).max()) + 1 if go.any() else 0
        azd, bzd, czd = az.astype(np.float64), bz.astype(np.float64), cz.astype(np.float64)
        for dj in range(H):
            for di in range(W):
                i, j = i0 + di, j0 + dj
                inside = go & (i <= i1) & (j <= j1)
                px, py = i.astype(np.float64), j.astype(np.float64)
                w0 = (cx - bx) * (py - by) - (cy - by) * (px - bx)
                w1 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx)
                w2 = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
                cov = inside & (((w0 >= 0.0) & (w1 >= 0.0) & (w2 >= 0.0)) | ((w0 <= 0.0) & (w1 <= 0.0) & (w2 <= 0.0)))
                zz = ((w0 * azd + w1 * bzd + w2 * czd) / area).astype(np.float32)
                cov &= np.isfinite(zz) & (zz > 0)
                if cov.any():
                    np.minimum.at(zbuf, j[cov] * cols + i[cov], zz[cov].view(np.uint32))
    return over, max(W, H)


def register(depth, dcam, ccam, c_rows, c_cols, R, t, *, depth_scale=0.001, z_min=0.0, z_max=0.0, quad_dz_abs=0.02,
             quad_dz_rel=0.02, ray_table=None):
    """ppf_depth_register: (image float32 [c_rows][c_cols], counters dict, info dict)"""
    rows, cols = depth.shape
    z, keep = kept_depth(depth, depth_scale, z_min, z_max)
    rt = rays(dcam, rows, cols) if ray_table is None else ray_table
    with np.errstate(all="ignore"):
        zd = z.astype(np.float64)
        P0, P1, P2 = rt[..., 0] * zd, rt[..., 1] * zd, zd
        Q = [R[r][0] * P0 + R[r][1] * P1 + R[r][2] * P2 + t[r] for r in range(3)]
        front = keep & ~np.isnan(rt[..., 0]) & (Q[2] > 0.0)
        uc, vc, ok = project(ccam, Q[0] / Q[2], Q[1] / Q[2])
        valid = front & ok
        zc = Q[2].astype(np.float32)
        n_vertices = int(valid.sum())
        zbuf = np.full(c_rows * c_cols, EMPTY, np.uint32)
        counters = dict(n_vertices=n_vertices, n_quads=0, n_quads_cut=0, n_quads_oversize=0)
        info = dict(max_box=0)
        if rows > 1 and cols > 1:
            sl = [(slice(0, -1), slice(0, -1)), (slice(0, -1), slice(1, None)), (slice(1, None), slice(0, -1)), (slice(1, None), slice(1, None))]
            V = [(uc[s].ravel(), vc[s].ravel(), zc[s].ravel()) for s in sl]       # v00 v10 v01 v11
            quad = valid[sl[0]].ravel() & valid[sl[1]].ravel() & valid[sl[2]].ravel() & valid[sl[3]].ravel()
            zs = np.stack([v[2] for v in V])
            lo, hi = zs.min(axis=0), zs.max(axis=0)
            cut = quad & (hi - lo > np.float32(quad_dz_abs) + np.float32(quad_dz_rel) * lo)
            tri = np.nonzero(quad & ~cut)[0]
            o1, m1 = _draw(zbuf, c_cols, c_rows, tri, V[0], V[1], V[2])
            o2, m2 = _draw(zbuf, c_cols, c_rows, tri, V[3], V[2], V[1])
            info["max_box"] = max(m1, m2)
            counters.update(n_quads=int(quad.sum()), n_quads_cut=int(cut.sum()), n_quads_oversize=int((o1 | o2).sum()))
    filled = zbuf != EMPTY
    img = np.where(filled, zbuf, np.uint32(0)).view(np.float32).reshape(c_rows, c_cols)
    counters["n_filled"] = int(filled.sum())
    return img, counters, info


# ---- scenes of the tests -------------------------------------------------------------------------------------------
PLANE_N, PLANE_D = (0.10, -0.05, 1.0), 0.8   # n . P = 0.8 in the depth frame


def plane_depth(dcam, rows, cols, n=PLANE_N, d=PLANE_D):
    """the depth image (float32 z) of the plane n . P = d: each depth pixel's ray (x, y, 1) z intersected with it"""
    rt = rays(dcam, rows, cols)
    return (d / (n[0] * rt[..., 0] + n[1] * rt[..., 1] + n[2])).astype(np.float32)


def plane_analytic(ccam, c_rows, c_cols, R, t, n=PLANE_N, d=PLANE_D):
    """the same plane's depth along each colour pixel's own ray (float64): Q = s (x, y, 1), n . R^T (Q - t) = d"""
    rt = rays(ccam, c_rows, c_cols)
    Rn = np.asarray(R) @ np.asarray(n)
    return (d + Rn @ np.asarray(t)) / (rt[..., 0] * Rn[0] + rt[..., 1] * Rn[1] + Rn[2])


BOX_RECT = (14, 34, 20, 44)   # depth pixel rows 14..33, columns 20..43


def plane_with_box(dcam, rows, cols, in_front=0.5):
    """the plane with a fronto-parallel box in_front metres before the plane's depth at the image centre"""
    z = plane_depth(dcam, rows, cols)
    r0, r1, c0, c1 = BOX_RECT
    z[r0:r1, c0:c1] = np.float32(PLANE_D - in_front)
    return z
