"""A numpy restatement of DESIGN.md §15: the surfel z-buffer of posed model rows, the visibility test of
ppf_verify_frame_rendered and the frame buffer of ppf_render_frame.  Every step is the fp64 / fp32 arithmetic the kernels
do, in the same order; the minima go through np.minimum.at, which does not depend on order either."""
import numpy as np

MAX_SPLAT = 8
EMPTY32 = np.uint32(0xFFFFFFFF)
EMPTY64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def move_np(model, T):
    """a numpy stand-in for ppf_transform_pc_pose (not its bits): for figures that need no device"""
    T = np.asarray(T, dtype=np.float64)
    p = model[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    n = model[:, 3:6].astype(np.float64) @ T[:3, :3].T
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return np.concatenate([p, n], axis=1).astype(np.float32)


def centre(o, intr):
    """(rendered, ui, vi): the rows that are drawn (finite, z > 0) and their centre pixels as doubles"""
    fx, fy, ppx, ppy = (float(v) for v in intr)
    with np.errstate(all="ignore"):
        x, y, z = (o[:, k].astype(np.float64) for k in range(3))
        ren = np.isfinite(o).all(axis=1) & (o[:, 2] > 0)
        ui = np.floor(x * fx / z + ppx + 0.5)
        vi = np.floor(y * fy / z + ppy + 0.5)
    return ren, ui, vi


def covers(o, rows, cols, intr, radius):
    """every (row, pixel, depth bits) a rendered row covers: (row index, v * cols + u, uint32 bits of (float)t)"""
    fx, fy, ppx, ppy = (float(v) for v in intr)
    r = float(np.float32(radius))
    ren, ui, vi = centre(o, intr)
    idx = np.nonzero(ren)[0]
    q = o[idx]
    x, y, z, nx, ny, nz = (q[:, k].astype(np.float64) for k in range(6))
    ui, vi = ui[idx], vi[idx]
    rx = np.minimum(float(MAX_SPLAT), np.ceil(r * fx / z))
    ry = np.minimum(float(MAX_SPLAT), np.ceil(r * fy / z))
    npd = (nx * x + ny * y) + nz * z
    out_i, out_p, out_d = [], [], []
    with np.errstate(all="ignore"):
        for dv in range(-MAX_SPLAT, MAX_SPLAT + 1):
            for du in range(-MAX_SPLAT, MAX_SPLAT + 1):
                u, v = ui + du, vi + dv
                ok = (abs(du) <= rx) & (abs(dv) <= ry) & (u >= 0) & (u < cols) & (v >= 0) & (v < rows)
                if not ok.any():
                    continue
                dx, dy = (u - ppx) / fx, (v - ppy) / fy
                den = (nx * dx + ny * dy) + nz
                t = npd / den
                ex, ey, ez = t * dx - x, t * dy - y, t - z
                ok &= (den != 0) & np.isfinite(t) & (t > 0) & ((ex * ex + ey * ey) + ez * ez <= r * r)
                k = np.nonzero(ok)[0]
                out_i.append(idx[k])
                out_p.append(v[k].astype(np.int64) * cols + u[k].astype(np.int64))
                out_d.append(t[k].astype(np.float32).view(np.uint32))
    cat = (lambda a, dt: np.concatenate(a) if a else np.zeros(0, dtype=dt))
    return cat(out_i, np.int64), cat(out_p, np.int64), cat(out_d, np.uint32)


def zbuffer(o, rows, cols, intr, radius):
    """the z-buffer of one pose: uint32 depth bits per pixel, EMPTY32 where nothing covers it"""
    zb = np.full(rows * cols, EMPTY32, dtype=np.uint32)
    _, p, d = covers(o, rows, cols, intr, radius)
    np.minimum.at(zb, p, d)
    return zb.reshape(rows, cols)


def visible(o, zb, intr, tol):
    """per row: drawn, its centre pixel in the image, and that pixel empty or z <= zbuf + tol (an fp32 add)"""
    rows, cols = zb.shape
    ren, ui, vi = centre(o, intr)
    inr = ren & (ui >= 0) & (ui < cols) & (vi >= 0) & (vi < rows)
    vis = np.zeros(len(o), dtype=bool)
    k = np.nonzero(inr)[0]
    b = zb[vi[k].astype(np.int64), ui[k].astype(np.int64)]
    with np.errstate(all="ignore"):
        near = o[k, 2] <= b.view(np.float32) + np.float32(tol)
    vis[k] = (b == EMPTY32) | near
    return vis


def facing(o):
    with np.errstate(all="ignore"):
        return (o[:, 3].astype(np.float64) * o[:, 0].astype(np.float64) + o[:, 4].astype(np.float64) * o[:, 1].astype(np.float64)) + \
            o[:, 5].astype(np.float64) * o[:, 2].astype(np.float64) < 0


def hidden_share(o, rows, cols, intr, radius, tol):
    """the share of finite camera-facing rows that the z-buffer of their own pose calls hidden"""
    f = np.isfinite(o).all(axis=1) & facing(o)
    vis = visible(o, zbuffer(o, rows, cols, intr, radius), intr, tol)
    return 1.0 - float((f & vis).sum()) / max(1, int(f.sum()))


def render_frame(moved, rows, cols, intr, radius):
    """ppf_render_frame: moved is a list of (detection index, moved rows); returns (depth, label)"""
    zb = np.full(rows * cols, EMPTY64, dtype=np.uint64)
    for i, o in moved:
        _, p, d = covers(o, rows, cols, intr, radius)
        np.minimum.at(zb, p, (d.astype(np.uint64) << np.uint64(32)) | np.uint64(i))
    empty = zb == EMPTY64
    depth = (zb >> np.uint64(32)).astype(np.uint32).view(np.float32)
    depth[empty] = 0
    label = (zb & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    label[empty] = -1
    return depth.reshape(rows, cols), label.reshape(rows, cols)
