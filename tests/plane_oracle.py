"""ppf_prep_planes / ppf_prep_planes_apply restated in numpy: integers, fp64 + - * / sqrt evaluated as
written and left to right, nothing fused, sums by one fixed tree.  The device is held to this byte for byte: the kept rows,
the labels and every info field, the doubles included."""
import math

import numpy as np

NONE, REMOVED, REJECTED = 0, 1, 2
NO_REFIT, REMOVE_BEHIND = 1, 2
DEFAULTS = dict(distance_threshold=0.005, n_hypotheses=256, seed=1, max_planes=1, min_inliers=100, min_inlier_share=0.10, flags=0)
# ppf_plane_info as the C compiler lays it out
INFO = np.dtype([("n", "<f8", 3), ("d", "<f8"), ("status", "<i4"), ("hypothesis", "<i4"), ("n_rows", "<i4"), ("n_hyp_inliers", "<i4"),
                 ("n_inliers", "<i4"), ("n_behind", "<i4"), ("refit", "<i4"), ("reserved", "<i4")])
M32 = 0xFFFFFFFF


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def mix(x):
    """the u32 finaliser, on a python int or a uint64 array holding u32 values"""
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def tsum(v):
    """the fixed-tree sum: pad with +0.0 to a multiple of 64, lane l of every 64 takes v[l] + v[l + offset] for offsets 32 ... 1,
    again on the results until one value is left"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size == 0:
        return 0.0
    while True:
        pad = (-v.size) % 64
        if pad:
            v = np.concatenate([v, np.zeros(pad)])
        v = v.reshape(-1, 64).copy()
        for off in (32, 16, 8, 4, 2, 1):
            v[:, :off] = v[:, :off] + v[:, off:2 * off]
        v = v[:, 0].copy()
        if v.size == 1:
            return float(v[0])


def _rotate(A, V, p, q):
    apq = A[p][q]
    if apq == 0.0:
        return
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    at = -theta if theta < 0 else theta
    t = 1.0 / (at + math.sqrt(theta * theta + 1.0))
    if theta < 0:
        t = -t
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    app, aqq = A[p][p], A[q][q]
    A[p][p] = app - t * apq
    A[q][q] = aqq + t * apq
    A[p][q] = A[q][p] = 0.0
    r = 3 - p - q
    arp, arq = A[r][p], A[r][q]
    A[r][p] = A[p][r] = c * arp - s * arq
    A[r][q] = A[q][r] = s * arp + c * arq
    for k in range(3):
        vkp, vkq = V[k][p], V[k][q]
        V[k][p] = c * vkp - s * vkq
        V[k][q] = s * vkp + c * vkq


def jacobi_normal(cov):
    """cov = (xx, xy, xz, yy, yz, zz): 12 cyclic sweeps over (0,1), (0,2), (1,2); the column of the smallest diagonal entry
    (strict <, in the order 0, 1, 2) divided by its length"""
    with np.errstate(all="ignore"):
        c = [float(v) for v in cov]
        A = [[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]
        V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
        for _ in range(12):
            _rotate(A, V, 0, 1)
            _rotate(A, V, 0, 2)
            _rotate(A, V, 1, 2)
        lam, col = A[0][0], 0
        if A[1][1] < lam:
            lam, col = A[1][1], 1
        if A[2][2] < lam:
            lam, col = A[2][2], 2
        nv = [V[0][col], V[1][col], V[2][col]]
        ln = math.sqrt(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2])
        return np.array([nv[0] / ln, nv[1] / ln, nv[2] / ln]) if ln != 0.0 else np.full(3, np.nan)


def signed(P, x, y, z):
    with np.errstate(all="ignore"):
        return ((P[0] * x + P[1] * y) + P[2] * z) + P[3]


def hypotheses(L, seed, r, H):
    """(H, 4) planes through three rows of L (fp64, m x 3) each, NaN rows where the hypothesis is invalid"""
    m = L.shape[0]
    base = mix((seed + 0x9E3779B9 * (r + 1)) & M32)
    h = np.arange(H, dtype=np.uint64)
    hh = mix(np.uint64(base) ^ h)
    idx = [((mix(hh ^ np.uint64(k)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64) for k in range(3)]
    with np.errstate(all="ignore"):
        a, b, c = L[idx[0]], L[idx[1]], L[idx[2]]
        e1, e2 = b - a, c - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ok = np.isfinite(l2) & (l2 > 0)
        n = n / np.sqrt(l2)[:, None]
        d = -((n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2])
        flip = d < 0
        n[flip] = -n[flip]
        d[flip] = -d[flip]
    P = np.concatenate([n, d[:, None]], axis=1)
    P[~ok] = np.nan
    return P


def refit(L, inl, k):
    """the plane through the inliers' centroid along the smallest eigenvector of their covariance; None if not finite"""
    x, y, z = L[:, 0], L[:, 1], L[:, 2]
    with np.errstate(all="ignore"):
        c = [tsum(np.where(inl, v, 0.0)) / k for v in (x, y, z)]
        d = [np.where(inl, v - ci, 0.0) for v, ci in zip((x, y, z), c)]
        cov = [tsum(np.where(inl, d[i] * d[j], 0.0)) / k for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        n = jacobi_normal(cov)
        dd = -((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2])
        if dd < 0:
            n, dd = -n, -dd
    P = np.array([n[0], n[1], n[2], dd])
    return P if np.isfinite(P).all() else None


def remove_planes(rows, p=None, curv=None):
    """rows: (n, 3) or (n, 6) float32.  Returns (kept rows, kept curvature or None, info (max_planes,) INFO, labels (n,) uint8)"""
    p = params(**(p or {}))
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n = rows.shape[0]
    thr = float(np.float32(p["distance_threshold"]))
    share = float(np.float32(p["min_inlier_share"]))
    info = np.zeros(p["max_planes"], dtype=INFO)
    labels = np.zeros(n, dtype=np.uint8)
    live = np.arange(n)
    xyz = rows[:, :3].astype(np.float64)
    finite = np.isfinite(xyz).all(axis=1)
    for r in range(p["max_planes"]):
        m = live.size
        if m < 3:
            break
        L = xyz[live]
        x, y, z = L[:, 0], L[:, 1], L[:, 2]
        P = hypotheses(L, p["seed"], r, p["n_hypotheses"])
        counts = np.zeros(p["n_hypotheses"], dtype=np.int64)
        for h in np.nonzero(~np.isnan(P[:, 3]))[0]:
            counts[h] = np.count_nonzero(np.abs(signed(P[h], x, y, z)) <= thr)
        h = int(np.argmax(counts))   # the first of the largest
        k0 = int(counts[h])
        row = info[r]
        valid = not np.isnan(P[h, 3])
        row["n"], row["d"] = (P[h, :3], P[h, 3]) if valid else (0.0, 0.0)
        row["hypothesis"], row["n_rows"], row["n_hyp_inliers"] = h, m, k0
        if k0 < p["min_inliers"] or float(k0) < share * float(m):
            row["status"] = REJECTED
            break
        row["status"] = REMOVED
        plane, k = P[h], k0
        if not p["flags"] & NO_REFIT:
            Q = refit(L, np.abs(signed(plane, x, y, z)) <= thr, float(k0))
            if Q is not None:
                k1 = int(np.count_nonzero(np.abs(signed(Q, x, y, z)) <= thr))
                if k1 >= k0:
                    plane, k = Q, k1
                    row["refit"] = 1
                    row["n"], row["d"] = Q[:3], Q[3]
        s = signed(plane, x, y, z)
        with np.errstate(all="ignore"):
            inl = np.abs(s) <= thr
            beh = (s < -thr) & finite[live] if p["flags"] & REMOVE_BEHIND else np.zeros(m, dtype=bool)
        row["n_inliers"], row["n_behind"] = k, int(beh.sum())
        assert int(inl.sum()) == k
        labels[live[inl]] = 1 + r
        labels[live[beh]] = 0x80 | (1 + r)
        live = live[~(inl | beh)]
    return rows[live], (None if curv is None else np.asarray(curv, dtype=np.float32)[live]), info, labels


def apply_planes(rows, info, p=None):
    """the rows that are neither inliers of a REMOVED plane of `info` nor, with REMOVE_BEHIND, behind one: the keep mask"""
    p = params(**(p or {}))
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    xyz = rows[:, :3].astype(np.float64)
    thr = float(np.float32(p["distance_threshold"]))
    keep = np.ones(rows.shape[0], dtype=bool)
    finite = np.isfinite(xyz).all(axis=1)
    for row in info:
        if row["status"] != REMOVED:
            continue
        s = signed([row["n"][0], row["n"][1], row["n"][2], row["d"]], xyz[:, 0], xyz[:, 1], xyz[:, 2])
        with np.errstate(all="ignore"):
            keep &= ~(np.abs(s) <= thr)
            if p["flags"] & REMOVE_BEHIND:
                keep &= ~((s < -thr) & finite)
    return keep
