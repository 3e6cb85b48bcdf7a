"""ppf_cloud_from_depth_normals restated in numpy, vectorised over the kept pixels: the rows of
ppf_cloud_from_depth with, per row, the normal and curvature of a plane fit over the pixel's image window.  fp64 + - * /
sqrt evaluated as written and left to right, nothing fused, every sum sequential over the neighbours only, in visiting order
(dv ascending, du ascending inside a row).  The device is held to this byte for byte, NaNs included."""
import numpy as np

DEFAULTS = dict(radius=3, max_depth_change=0.02, min_neighbours=3, drop=False)
MAX_RADIUS = 8


def metric_depth(depth, depth_scale=0.001):
    depth = np.asarray(depth)
    return depth if depth.dtype == np.float32 else (depth.astype(np.float64) * depth_scale).astype(np.float32)


def keep_mask(z, z_min=0.0, z_max=0.0):
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0) & (z >= np.float32(z_min)) & ((np.float32(z_max) == 0) | (z <= np.float32(z_max)))


def back_project_axis(idx, pp, f, z, fp64):
    """depth_back_project for integer pixel coordinates idx (broadcast against the float32 image z) -> float32"""
    with np.errstate(all="ignore"):
        if fp64:
            return ((idx - pp) * z.astype(np.float64) / f).astype(np.float32)
        return (((idx - pp).astype(np.float32) * z).astype(np.float64) / f).astype(np.float32)


def _rotate(A, V, p, q):
    apq = A[p][q]
    on = apq != 0.0
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    neg = theta < 0
    at = np.where(neg, -theta, theta)
    t = 1.0 / (at + np.sqrt(theta * theta + 1.0))
    t = np.where(neg, -t, t)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    app, aqq = A[p][p], A[q][q]
    r = 3 - p - q
    arp, arq = A[r][p], A[r][q]
    A[p][p] = np.where(on, app - t * apq, app)
    A[q][q] = np.where(on, aqq + t * apq, aqq)
    A[p][q] = A[q][p] = np.where(on, 0.0, apq)
    A[r][p] = A[p][r] = np.where(on, c * arp - s * arq, arp)
    A[r][q] = A[q][r] = np.where(on, s * arp + c * arq, arq)
    for k in range(3):
        vkp, vkq = V[k][p], V[k][q]
        V[k][p] = np.where(on, c * vkp - s * vkq, vkp)
        V[k][q] = np.where(on, s * vkp + c * vkq, vkq)


def smallest_eigvec(cov):
    """prep_smallest_eigvec elementwise on six fp64 arrays (xx, xy, xz, yy, yz, zz): (lam, [n0, n1, n2])"""
    n = cov[0].shape[0]
    A = [[cov[0], cov[1], cov[2]], [cov[1], cov[3], cov[4]], [cov[2], cov[4], cov[5]]]
    V = [[np.full(n, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    for _ in range(12):
        _rotate(A, V, 0, 1)
        _rotate(A, V, 0, 2)
        _rotate(A, V, 1, 2)
    lam = A[0][0]
    nv = [V[0][0], V[1][0], V[2][0]]
    for col in (1, 2):
        less = A[col][col] < lam
        lam = np.where(less, A[col][col], lam)
        nv = [np.where(less, V[i][col], nv[i]) for i in range(3)]
    ln = np.sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2])
    return lam, [nv[0] / ln, nv[1] / ln, nv[2] / ln]


def window_offsets(radius):
    return [(dv, du) for dv in range(-radius, radius + 1) for du in range(-radius, radius + 1)]


def depth_normals(depth, intr, *, depth_scale=0.001, z_min=0.0, z_max=0.0, fp64=False, radius=3, max_depth_change=0.02,
                  min_neighbours=3, drop=False, return_k=False):
    """(rows (N, 6) float32, curvature (N,) float32[, k (N,) int64 before any drop]) of the kept pixels in row-major order"""
    fx, fy, ppx, ppy = [float(v) for v in intr]
    r = int(radius)
    z = metric_depth(depth, depth_scale)
    H, W = z.shape
    keep = keep_mask(z, z_min, z_max)
    x = back_project_axis(np.arange(W)[None, :], ppx, fx, z, fp64)
    y = back_project_axis(np.arange(H)[:, None], ppy, fy, z, fp64)
    pad = lambda a, fill: np.pad(a, r, constant_values=fill)  # noqa: E731
    Kp, Xp, Yp, Zp = pad(keep, False), pad(x, 0), pad(y, 0), pad(z, 0)
    vv, uu = np.nonzero(keep)
    n = vv.size
    px, py, pz = x[vv, uu], y[vv, uu], z[vv, uu]
    with np.errstate(all="ignore"):
        zp = pz.astype(np.float64)
        lim = np.float64(np.float32(max_depth_change)) * zp

        def neighbours():
            for dv, du in window_offsets(r):
                iv, iu = vv + (r + dv), uu + (r + du)
                zq = Zp[iv, iu].astype(np.float64)
                nb = Kp[iv, iu] & (np.abs(zq - zp) <= lim)
                yield nb, Xp[iv, iu].astype(np.float64), Yp[iv, iu].astype(np.float64), zq

        k = np.zeros(n, np.int64)
        c = [np.zeros(n), np.zeros(n), np.zeros(n)]
        for nb, qx, qy, qz in neighbours():
            k += nb
            for a, q in enumerate((qx, qy, qz)):
                c[a] = np.where(nb, c[a] + q, c[a])
        kd = k.astype(np.float64)
        c = [v / kd for v in c]
        cov = [np.zeros(n) for _ in range(6)]
        for nb, qx, qy, qz in neighbours():
            d = (qx - c[0], qy - c[1], qz - c[2])
            for a, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                cov[a] = np.where(nb, cov[a] + d[i] * d[j], cov[a])
        cov = [v / kd for v in cov]
        trace = (cov[0] + cov[3]) + cov[5]
        lam, nv = smallest_eigvec(cov)
        cos_theta = -((px.astype(np.float64) * nv[0] + py.astype(np.float64) * nv[1]) + pz.astype(np.float64) * nv[2])
        flip = cos_theta < 0
        nv = [np.where(flip, -v, v) for v in nv]
        curv = np.where(trace != 0.0, (np.abs(lam) / np.abs(trace)).astype(np.float32), np.float32(0)).astype(np.float32)
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2] = px, py, pz
    for a in range(3):
        rows[:, 3 + a] = nv[a].astype(np.float32)
    none = k < int(min_neighbours)
    rows[none, 3:] = np.float32(np.nan)
    curv[none] = np.float32(np.nan)
    if drop:
        rows, curv = rows[~none], curv[~none]
    return (rows, curv, k) if return_k else (rows, curv)
