"""ppf_depth_edges restated in numpy: the occluding, occluded and boundary edges of a depth image, and the
edge cloud they select.  The jump test is one fp64 expression evaluated as written, nothing fused, and the walk is a first-hit
search along eight rays, so there is one right answer and the device is held to it byte for byte.  Two implementations:
``edges`` advances all pixels of a direction together, one step of the walk at a time; ``edges_loops`` walks pixel by pixel in
Python doubles."""
import numpy as np

import depth_normals_oracle as N

OCCLUDING, OCCLUDED, BOUNDARY, CURVATURE = 1, 2, 4, 8
ALL = 15
MAX_GAP = 8
DEFAULTS = dict(depth_abs=0.02, depth_quad=0.0, max_gap=2, curvature_threshold=0.03, select=OCCLUDING | BOUNDARY | CURVATURE, flags=0)
DIRECTIONS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
STAT_KEYS = ("n_kept", "n_occluding", "n_occluded", "n_boundary", "n_curvature", "n_edge", "n_selected", "n_no_normal", "n_rows")


def _f32(v):
    return np.float64(np.float32(v))


def _check(depth_abs, depth_quad, max_gap, curvature_threshold, select, flags):
    ok = (np.isfinite(depth_abs) and depth_abs >= 0 and np.isfinite(depth_quad) and depth_quad >= 0 and 0 <= max_gap <= MAX_GAP
          and curvature_threshold >= 0 and select != 0 and not (select & ~ALL) and flags == 0)
    if not ok:
        raise ValueError("an edge parameter is outside its range")


def jump(zp, zq, depth_abs, depth_quad):
    """fabs(Zq - Zp) > (double)depth_abs + (double)depth_quad * (Zp * Zq) on float64 arrays or scalars"""
    return np.abs(zq - zp) > _f32(depth_abs) + _f32(depth_quad) * (zp * zq)


def _curvature_bits(kept, normals, curvature_threshold):
    """(the CURVATURE bit image, per pixel whether its normal is finite) from the normals cloud of the kept pixels"""
    rows, curv = normals
    rows, curv = np.asarray(rows, np.float32), np.asarray(curv, np.float32)
    if rows.shape[0] != int(kept.sum()) or curv.shape[0] != rows.shape[0]:
        raise ValueError(f"the normals cloud has {rows.shape[0]} rows, the image keeps {int(kept.sum())} pixels")
    bit = np.zeros(kept.shape, np.uint8)
    finite = np.zeros(kept.shape, bool)
    with np.errstate(invalid="ignore"):
        bit[kept] = np.where(curv > np.float32(curvature_threshold), CURVATURE, 0).astype(np.uint8)
    finite[kept] = np.isfinite(rows[:, 3:6]).all(axis=1)
    return bit, finite


def _finish(mask, z, kept, normals, finite, intr, fp64, select):
    sel = (mask & select) != 0
    stats = dict(n_kept=int(kept.sum()), n_occluding=int(((mask & OCCLUDING) != 0).sum()), n_occluded=int(((mask & OCCLUDED) != 0).sum()),
                 n_boundary=int(((mask & BOUNDARY) != 0).sum()), n_curvature=int(((mask & CURVATURE) != 0).sum()),
                 n_edge=int((mask != 0).sum()), n_selected=int(sel.sum()), n_no_normal=0, n_rows=0)
    cloud = None
    if normals is not None:
        rows, curv = np.asarray(normals[0], np.float32), np.asarray(normals[1], np.float32)
        index = np.full(mask.shape, -1, np.int64)
        index[kept] = np.arange(rows.shape[0])
        take = index[sel & finite]
        stats["n_no_normal"] = int((sel & ~finite).sum())
        cloud = (rows[take].copy(), curv[take].copy())
    elif intr is not None:
        fx, fy, ppx, ppy = [float(v) for v in intr]
        vv, uu = np.nonzero(sel)
        zs = z[vv, uu]
        rows = np.zeros((vv.size, 6), np.float32)
        rows[:, 0] = N.back_project_axis(uu, ppx, fx, zs, fp64)
        rows[:, 1] = N.back_project_axis(vv, ppy, fy, zs, fp64)
        rows[:, 2] = zs
        cloud = (rows, np.zeros(vv.size, np.float32))
    if cloud is not None:
        stats["n_rows"] = int(cloud[0].shape[0])
    return mask, cloud, stats


def edges(depth, intr=None, *, depth_scale=0.001, z_min=0.0, z_max=0.0, fp64=False, normals=None, depth_abs=0.02, depth_quad=0.0,
          max_gap=2, curvature_threshold=0.03, select=OCCLUDING | BOUNDARY | CURVATURE, flags=0):
    """(mask uint8 image, cloud (rows (n, 6), curvature (n,)) or None, stats).  normals: None or (rows (n_kept, 6), curvature
    (n_kept,)) as ppf_cloud_from_depth_normals gives them; the cloud is None without normals and without intr"""
    _check(depth_abs, depth_quad, max_gap, curvature_threshold, select, flags)
    z = N.metric_depth(depth, depth_scale)
    kept = N.keep_mask(z, z_min, z_max)
    H, W = z.shape
    h = max_gap + 1
    # the padded planes: state 0 outside the image, 1 not kept, 2 kept
    state = np.zeros((H + 2 * h, W + 2 * h), np.uint8)
    state[h:h + H, h:h + W] = np.where(kept, 2, 1)
    Zp = np.zeros(state.shape, np.float64)
    Zp[h:h + H, h:h + W] = np.where(kept, z, 0).astype(np.float64)
    Z = Zp[h:h + H, h:h + W]
    mask = np.zeros((H, W), np.uint8)
    for dv, du in DIRECTIONS:
        view = lambda a, j: a[h + j * dv:h + j * dv + H, h + j * du:h + j * du + W]  # noqa: E731
        walking = kept & (view(state, 1) != 0)
        for j in range(1, h + 1):
            s, zq = view(state, j), view(Zp, j)
            left = walking & (s == 0)
            mask[left] |= BOUNDARY
            hit = walking & (s == 2)
            with np.errstate(all="ignore"):
                jm = hit & jump(Z, zq, depth_abs, depth_quad)
            mask[jm & (zq > Z)] |= OCCLUDING
            mask[jm & (zq < Z)] |= OCCLUDED
            walking = walking & (s == 1)
        mask[walking] |= BOUNDARY
    finite = None
    if normals is not None:
        bit, finite = _curvature_bits(kept, normals, curvature_threshold)
        mask |= bit
    return _finish(mask, z, kept, normals, finite, intr, fp64, select)


def edges_loops(depth, intr=None, *, depth_scale=0.001, z_min=0.0, z_max=0.0, fp64=False, normals=None, depth_abs=0.02, depth_quad=0.0,
                max_gap=2, curvature_threshold=0.03, select=OCCLUDING | BOUNDARY | CURVATURE, flags=0):
    """the same, pixel by pixel and direction by direction as the specification words it"""
    _check(depth_abs, depth_quad, max_gap, curvature_threshold, select, flags)
    z = N.metric_depth(depth, depth_scale)
    kept = N.keep_mask(z, z_min, z_max)
    H, W = z.shape
    A, Q = float(_f32(depth_abs)), float(_f32(depth_quad))
    mask = np.zeros((H, W), np.uint8)
    for v in range(H):
        for u in range(W):
            if not kept[v, u]:
                continue
            zp = float(z[v, u])
            m = 0
            for dv, du in DIRECTIONS:
                if not (0 <= v + dv < H and 0 <= u + du < W):
                    continue
                got = BOUNDARY
                for j in range(1, max_gap + 2):
                    qv, qu = v + j * dv, u + j * du
                    if not (0 <= qv < H and 0 <= qu < W):
                        break
                    if kept[qv, qu]:
                        zq = float(z[qv, qu])
                        got = 0
                        if abs(zq - zp) > A + Q * (zp * zq):
                            got = OCCLUDING if zq > zp else (OCCLUDED if zq < zp else 0)
                        break
                m |= got
            mask[v, u] = m
    finite = None
    if normals is not None:
        bit, finite = _curvature_bits(kept, normals, curvature_threshold)
        mask |= bit
    return _finish(mask, z, kept, normals, finite, intr, fp64, select)


def same(a, b):
    """two results equal byte for byte: the mask, the cloud's rows and curvatures, every count"""
    if a[0].tobytes() != b[0].tobytes() or a[0].shape != b[0].shape or a[2] != b[2] or (a[1] is None) != (b[1] is None):
        return False
    return a[1] is None or (a[1][0].tobytes() == b[1][0].tobytes() and a[1][1].tobytes() == b[1][1].tobytes())
