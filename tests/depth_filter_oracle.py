"""ppf_depth_filter restated in numpy, vectorised over the image: the support test on the 8 neighbours, then
the two Tukey biweights over the (2 radius + 1)^2 window of the supported pixels.  fp64 + - * / evaluated as written and left
to right, nothing fused; the taps are visited in the specified order (dv ascending, du ascending inside a row) and every
pixel's two sums grow elementwise in that order.  The parameters are the float32 values the C record holds, widened.  The
device is held to this byte for byte."""
import numpy as np

from depth_normals_oracle import keep_mask, metric_depth

DEFAULTS = dict(radius=3, range_abs=0.01, range_quad=0.0, support_abs=0.01, support_quad=0.0, min_support=6)
MAX_RADIUS = 8
NEIGHBOURS = [(dv, du) for dv in (-1, 0, 1) for du in (-1, 0, 1) if (dv, du) != (0, 0)]


def _f32(v):
    return np.float64(np.float32(v))


def supported_mask(z, keep, support_abs, support_quad, min_support):
    """step 1: the kept pixels with at least min_support supporting neighbours (a neighbour outside the image supports)"""
    H, W = z.shape
    Z = z.astype(np.float64)
    Zq = np.pad(Z, 1, constant_values=np.nan)
    Kq = np.pad(keep, 1, constant_values=False)
    outside = np.pad(np.zeros((H, W), bool), 1, constant_values=True)
    with np.errstate(all="ignore"):
        S = _f32(support_abs) + _f32(support_quad) * (Z * Z)
        count = np.zeros((H, W), np.int64)
        for dv, du in NEIGHBOURS:
            sl = (slice(1 + dv, 1 + dv + H), slice(1 + du, 1 + du + W))
            count += outside[sl] | (Kq[sl] & (np.abs(Zq[sl] - Z) <= S))
    return keep & ((int(min_support) == 0) | (count >= int(min_support)))


def filter_depth(depth, *, depth_scale=0.001, z_min=0.0, z_max=0.0, radius=3, range_abs=0.01, range_quad=0.0, support_abs=0.01,
                 support_quad=0.0, min_support=6):
    """(out (rows, cols) float32, dict(n_kept, n_unsupported, n_written))"""
    r = int(radius)
    z = metric_depth(depth, depth_scale)
    H, W = z.shape
    keep = keep_mask(z, z_min, z_max)
    sup = supported_mask(z, keep, support_abs, support_quad, min_support)
    Z = z.astype(np.float64)
    Zs = np.pad(np.where(sup, Z, np.nan), r, constant_values=np.nan)   # NaN: not supported or outside the image
    D = np.float64((r + 1) * (r + 1))
    num, den = np.zeros((H, W)), np.zeros((H, W))
    with np.errstate(all="ignore"):
        R = _f32(range_abs) + _f32(range_quad) * (Z * Z)
        for dv in range(-r, r + 1):
            for du in range(-r, r + 1):
                s = 1.0 - np.float64(du * du + dv * dv) / D
                if not s > 0:
                    continue
                Zq = Zs[r + dv:r + dv + H, r + du:r + du + W]
                t = (Zq - Z) / R
                k = 1.0 - t * t
                ok = k > 0                                           # a NaN Zq fails
                w = (s * s) * (k * k)
                num = np.where(ok, num + w * Zq, num)
                den = np.where(ok, den + w, den)
        out = np.where(sup, (num / den).astype(np.float32), np.float32(0)).astype(np.float32)
    n_kept, n_written = int(keep.sum()), int(sup.sum())
    return out, dict(n_kept=n_kept, n_unsupported=n_kept - n_written, n_written=n_written)


def filter_depth_loops(depth, *, depth_scale=0.001, z_min=0.0, z_max=0.0, radius=3, range_abs=0.01, range_quad=0.0,
                       support_abs=0.01, support_quad=0.0, min_support=6):
    """the specification once more, pixel by pixel in Python doubles: what the vectorised form above is held to"""
    r = int(radius)
    z = metric_depth(depth, depth_scale)
    H, W = z.shape
    keep = keep_mask(z, z_min, z_max)
    sa, sq, ra, rq = (float(np.float32(v)) for v in (support_abs, support_quad, range_abs, range_quad))
    sup = np.zeros((H, W), bool)
    for v in range(H):
        for u in range(W):
            if not keep[v, u]:
                continue
            Zp = float(z[v, u])
            S = sa + sq * (Zp * Zp)
            count = 0
            for dv, du in NEIGHBOURS:
                qv, qu = v + dv, u + du
                if qv < 0 or qv >= H or qu < 0 or qu >= W:
                    count += 1
                elif keep[qv, qu] and abs(float(z[qv, qu]) - Zp) <= S:
                    count += 1
            sup[v, u] = int(min_support) == 0 or count >= int(min_support)
    out = np.zeros((H, W), np.float32)
    D = float((r + 1) * (r + 1))
    for v in range(H):
        for u in range(W):
            if not sup[v, u]:
                continue
            Zp = float(z[v, u])
            R = ra + rq * (Zp * Zp)
            num = den = 0.0
            for dv in range(-r, r + 1):
                for du in range(-r, r + 1):
                    qv, qu = v + dv, u + du
                    if qv < 0 or qv >= H or qu < 0 or qu >= W or not sup[qv, qu]:
                        continue
                    s = 1.0 - float(du * du + dv * dv) / D
                    if not s > 0:
                        continue
                    Zq = float(z[qv, qu])
                    t = (Zq - Zp) / R
                    k = 1.0 - t * t
                    if not k > 0:
                        continue
                    w = (s * s) * (k * k)
                    num = num + w * Zq
                    den = den + w
            out[v, u] = np.float32(num / den)
    n_kept, n_written = int(keep.sum()), int(sup.sum())
    return out, dict(n_kept=n_kept, n_unsupported=n_kept - n_written, n_written=n_written)
