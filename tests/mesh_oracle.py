"""The specification of ppf_cloud_from_mesh (include/ppf_hip.h) restated in numpy: every expression in fp64 in
the order the header writes it, the hash in integer arithmetic, the depth maps as unsigned minima of float bit patterns.
The device holds rows, counts and stats to this byte for byte; `area` alone is compared to 1e-12 (its summation order is free)."""
import numpy as np

N_VIEWS = 26
SMALL_PX = 16  # a clamped box of at most this many pixels a side takes the device's small path (n_large counts the others)
EMPTY = np.uint32(0xFFFFFFFF)
_M32 = np.uint64(0xFFFFFFFF)


class MeshCapacity(Exception):
    """more rows than max_rows: PPF_ERR_CAPACITY"""


def mix(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def mesh_hash(seed, k, c):
    """h(seed, k, c) as uint64 arrays holding 32-bit values"""
    s = mix((np.uint64(int(seed) & 0xFFFFFFFF) + np.uint64(0x9E3779B9)) & _M32)
    return mix(mix(s ^ (np.asarray(k, dtype=np.uint64) & _M32)) ^ (np.asarray(c, dtype=np.uint64) & _M32))


def fkey(f):
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def fkey_inv(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def norm(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def view_frames():
    """d, a, b of the 26 views, each (26, 3) float64"""
    d = []
    for x in (-1, 0, 1):
        for y in (-1, 0, 1):
            for z in (-1, 0, 1):
                nz = (x != 0) + (y != 0) + (z != 0)
                if nz:
                    s = 1.0 / np.sqrt(np.float64(nz))
                    d.append([np.float64(x) * s, np.float64(y) * s, np.float64(z) * s])
    d = np.array(d, dtype=np.float64)
    e = np.zeros_like(d)
    e[np.arange(N_VIEWS), np.argmin(np.abs(d), axis=1)] = 1.0  # argmin: the first on ties
    t = cross(d, e)
    a = t / norm(t)[:, None]
    return d, a, cross(d, a)


def triangles_geom(V, T):
    """v0, e1, e2, c, L, live of every triangle"""
    with np.errstate(all="ignore"):
        P = V[:, :3].astype(np.float64)
        v0, e1, e2 = P[T[:, 0]], P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]]
        c = cross(e1, e2)
        L = norm(c)
        live = (L > 0) & np.isfinite(L)
    return v0, e1, e2, c, L, live


def row_counts(L, live, spacing, seed, max_rows=0):
    """n_k of every triangle (0 where it is degenerate) and q; raises MeshCapacity"""
    cap = np.float64(max_rows if max_rows else 1 << 24)
    s = np.float64(np.float32(spacing))
    with np.errstate(all="ignore"):
        q = np.where(live, (0.5 * L) / (s * s), 0.0)
    if (q[live] >= cap).any() or not np.isfinite(q[live]).all():
        raise MeshCapacity()
    f = np.floor(q)
    thr = np.floor((q - f) * 16777216.0).astype(np.uint64)
    up = (mesh_hash(seed, np.arange(len(L)), 0) >> np.uint64(8)) < thr
    n = np.where(live, f.astype(np.int64) + up, 0)
    if n.sum() > cap:
        raise MeshCapacity()
    return n, q


def view_setup(V, T, live, map_size=0, depth_tol=0.0):
    R = int(map_size) if map_size else 256
    d, a, b = view_frames()
    if live.any():
        keys = fkey(V[T[live]].reshape(-1, V.shape[1])[:, :3])
        lo = fkey_inv(keys.min(axis=0)).astype(np.float64)
        hi = fkey_inv(keys.max(axis=0)).astype(np.float64)
        ctr = 0.5 * (lo + hi)
        g = hi - lo
        r = 0.5 * np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    else:
        ctr, r = np.zeros(3), np.float64(0.0)
    px = 2.0 * r / np.float64(R - 2)
    tol = np.float64(np.float32(depth_tol)) if depth_tol > 0 else 2.0 * px
    return dict(R=R, d=d, a=a, b=b, ctr=ctr, r=r, px=px, tol=tol, half=0.5 * np.float64(R))


def project(W, v, P):
    s = P - W["ctr"]
    X = dot(s, W["a"][v]) / W["px"] + W["half"]
    Y = dot(s, W["b"][v]) / W["px"] + W["half"]
    D = dot(s, W["d"][v]) + W["r"]
    return X, Y, D


def draw_maps(V, T, live, W):
    """the 26 depth maps (26, R, R) uint32, the clamped boxes' sides (26, n_triangles, 2) (0: nothing drawn) and n_large"""
    R = W["R"]
    maps = np.full((N_VIEWS, R, R), EMPTY, dtype=np.uint32)
    sides = np.zeros((N_VIEWS, len(T), 2), dtype=np.int64)
    idx = np.nonzero(live)[0]
    P = V[:, :3].astype(np.float64)
    n_large = 0
    if not len(idx):
        return maps, sides, 0
    for v in range(N_VIEWS):
        pr = [project(W, v, P[T[idx, c]]) for c in range(3)]
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = [(X, Y, D.astype(np.float32).astype(np.float64)) for X, Y, D in pr]
        x0 = np.maximum(np.ceil(np.minimum(np.minimum(ax, bx), cx)), 0.0)
        x1 = np.minimum(np.floor(np.maximum(np.maximum(ax, bx), cx)), np.float64(R - 1))
        y0 = np.maximum(np.ceil(np.minimum(np.minimum(ay, by), cy)), 0.0)
        y1 = np.minimum(np.floor(np.maximum(np.maximum(ay, by), cy)), np.float64(R - 1))
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        ok = (x1 >= x0) & (y1 >= y0) & (area != 0.0)
        i0, j0 = x0[ok].astype(np.int64), y0[ok].astype(np.int64)
        w, h = x1[ok].astype(np.int64) - i0 + 1, y1[ok].astype(np.int64) - j0 + 1
        sides[v, idx[ok], 0], sides[v, idx[ok], 1] = w, h
        n_large += int(((w > SMALL_PX) | (h > SMALL_PX)).sum())
        tri = [arr[ok] for arr in (ax, ay, az, bx, by, bz, cx, cy, cz, area)]
        flat = maps[v].reshape(-1)

        def pixels(sel, i, j):
            """draw pixels (i, j) of the triangles sel (index arrays of equal length)"""
            tax, tay, taz, tbx, tby, tbz, tcx, tcy, tcz, tar = [arr[sel] for arr in tri]
            fx, fy = i.astype(np.float64), j.astype(np.float64)
            w0 = (tcx - tbx) * (fy - tby) - (tcy - tby) * (fx - tbx)
            w1 = (tax - tcx) * (fy - tcy) - (tay - tcy) * (fx - tcx)
            w2 = (tbx - tax) * (fy - tay) - (tby - tay) * (fx - tax)
            cov = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
            z = (((w0 * taz + w1 * tbz) + w2 * tcz) / tar).astype(np.float32)
            z = np.where(z > 0, z, np.float32(0.0)).astype(np.float32)
            np.minimum.at(flat, (j * R + i)[cov], z.view(np.uint32)[cov])

        small = np.nonzero((w <= 32) & (h <= 32))[0]
        if len(small):
            for dj in range(int(h[small].max())):
                for di in range(int(w[small].max())):
                    m = small[(di < w[small]) & (dj < h[small])]
                    if len(m):
                        pixels(m, i0[m] + di, j0[m] + dj)
        for t in np.nonzero((w > 32) | (h > 32))[0]:
            jj, ii = np.meshgrid(np.arange(j0[t], j0[t] + h[t]), np.arange(i0[t], i0[t] + w[t]), indexing="ij")
            pixels(np.full(ii.size, t), ii.reshape(-1), jj.reshape(-1))
    return maps, sides, n_large


def mesh_sample(vertices, triangles, spacing, *, seed=0, normals=0, normal_offset=-1, visibility=1, map_size=0, min_views=0,
                depth_tol=0.0, orient=1, max_rows=0):
    """rows (n, 6) float32 and what the tests look at: stats (the entry's record, launches and waits excepted), tri (each
    output row's triangle), sampled (every sampled row before the visibility test), sampled_tri, keep, seen, sides, q, n_k"""
    V = np.ascontiguousarray(vertices, dtype=np.float32)
    T = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    v0, e1, e2, c, L, live = triangles_geom(V, T)
    n_k, q = row_counts(L, live, spacing, seed, max_rows)
    total = int(n_k.sum())
    k = np.repeat(np.arange(len(T)), n_k)
    j = np.arange(total) - np.repeat(np.cumsum(n_k) - n_k, n_k)
    u = ((mesh_hash(seed, k, 2 * j + 1) >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    w = ((mesh_hash(seed, k, 2 * j + 2) >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    swap = u + w > 1.0
    u, w = np.where(swap, 1.0 - u, u), np.where(swap, 1.0 - w, w)
    p = ((v0[k] + u[:, None] * e1[k]) + w[:, None] * e2[k]).astype(np.float32)
    with np.errstate(all="ignore"):
        n = (c[k] / L[k][:, None]).astype(np.float32)
        if normals == 1:
            N = V[:, normal_offset:normal_offset + 3].astype(np.float64)
            n0, n1, n2 = N[T[k, 0]], N[T[k, 1]], N[T[k, 2]]
            bw = (1.0 - u) - w
            m = (bw[:, None] * n0 + u[:, None] * n1) + w[:, None] * n2
            ln = norm(m)
            good = (ln > 0) & np.isfinite(ln)
            n = np.where(good[:, None], (m / ln[:, None]).astype(np.float32), n)
    rows = np.concatenate([p, n], axis=1).astype(np.float32).reshape(total, 6)
    sampled = rows.copy()
    stats = dict(n_triangles=len(T), n_degenerate=int((~live).sum()), n_sampled=total, n_flipped=0, n_large=0,
                 area=float(np.sum(0.5 * L[live])))
    keep, seen, sides = np.ones(total, dtype=bool), None, None
    if visibility:
        W = view_setup(V, T, live, map_size, depth_tol)
        maps, sides, stats["n_large"] = draw_maps(V, T, live, W)
        R = W["R"]
        seen, front, back = (np.zeros(total, dtype=np.int64) for _ in range(3))
        P, Nn = rows[:, :3].astype(np.float64), rows[:, 3:].astype(np.float64)
        with np.errstate(all="ignore"):
            for v in range(N_VIEWS):
                X, Y, D = project(W, v, P)
                fi, fj = np.floor(X + 0.5), np.floor(Y + 0.5)
                inside = (fi >= 0) & (fi <= R - 1) & (fj >= 0) & (fj <= R - 1)
                ii, jj = np.where(inside, fi, 0).astype(np.int64), np.where(inside, fj, 0).astype(np.int64)
                zb = maps[v, jj, ii]
                z = zb.view(np.float32).astype(np.float64)
                vis = ~inside | (zb == EMPTY) | (D.astype(np.float32).astype(np.float64) <= z + W["tol"])
                s = dot(Nn, W["d"][v])
                seen += vis
                front += vis & (s < 0)
                back += vis & (s > 0)
        keep = seen >= max(1, int(min_views))
        flip = keep & bool(orient) & (back > front)
        rows[flip, 3:] = -rows[flip, 3:]
        stats["n_flipped"] = int(flip.sum())
    out = np.ascontiguousarray(rows[keep])
    stats["n_rows"] = len(out)
    stats["n_hidden"] = total - len(out)
    return dict(rows=out, tri=k[keep], stats=stats, sampled=sampled, sampled_tri=k, keep=keep, seen=seen, sides=sides, q=q, n_k=n_k)
