"""ppf_depth_segments restated in numpy: the connected surfaces of a depth image in image space.  Every
comparison is an fp64 expression evaluated as written, nothing fused; a component is a set and its rank is by integers, so
there is one right answer and the device is held to it byte for byte.  Two implementations that share the pixels' classes and the final ranking:
``segments`` evaluates the link predicates vectorised per direction and joins them with a union-find; ``segments_bfs`` walks
the pixels one by one in Python doubles and grows each component breadth first."""
from collections import deque

import numpy as np

import depth_normals_oracle as N

DEFAULTS = dict(depth_abs=0.005, depth_quad=0.0, normal_cos=0.9659258, curvature_threshold=0.03, min_size=100, max_size=0,
                max_segments=64, flags=0)
EIGHT, UNORIENTED = 1, 2
MAX_SEGMENTS = 256
FORWARD4 = ((0, 1), (1, 0))                       # (dv, du): right, down
FORWARD8 = ((0, 1), (1, -1), (1, 0), (1, 1))
AROUND4 = ((-1, 0), (0, -1), (0, 1), (1, 0))      # ascending pixel index
AROUND8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def _f32(v):
    return np.float64(np.float32(v))


def classify(depth, normals, depth_scale, z_min, z_max, curvature_threshold):
    """z (float32 image), kept, eligible, smooth (bool images), nrm ((rows, cols, 3) float32 or None)"""
    z = N.metric_depth(depth, depth_scale)
    kept = N.keep_mask(z, z_min, z_max)
    if normals is None:
        return z, kept, kept.copy(), kept.copy(), None
    rows, curv = normals
    rows, curv = np.asarray(rows, np.float32), np.asarray(curv, np.float32)
    if rows.shape[0] != int(kept.sum()) or curv.shape[0] != rows.shape[0]:
        raise ValueError(f"the normals cloud has {rows.shape[0]} rows, the image keeps {int(kept.sum())} pixels")
    nrm = np.zeros(z.shape + (3,), np.float32)
    cv = np.full(z.shape, np.float32(np.nan))
    nrm[kept] = rows[:, 3:6]
    cv[kept] = curv
    eligible = kept & np.isfinite(nrm).all(axis=2)
    with np.errstate(invalid="ignore"):
        smooth = eligible & (cv <= np.float32(curvature_threshold))
    return z, kept, eligible, smooth, nrm


def _finish(z, kept, eligible, smooth, comp, attached, min_size, max_size, max_segments):
    """comp: per pixel the component's first (smallest smooth) pixel or -1; attached: the border pixels among them"""
    rows, cols = z.shape
    flat = comp.reshape(-1)
    firsts, sizes = np.unique(flat[flat >= 0], return_counts=True)
    valid = (sizes >= min_size) & ((max_size == 0) | (sizes <= max_size))
    order = sorted(range(len(firsts)), key=lambda i: (-int(sizes[i]), int(firsts[i])))
    ranked = [i for i in order if valid[i]][:max_segments]
    labels = np.full(z.shape, -1, np.int32)
    info = []
    for rank, i in enumerate(ranked):
        m = comp == firsts[i]
        labels[m] = rank
        vs, us = np.nonzero(m)
        info.append(dict(n_pixels=int(sizes[i]), n_border=int((m & attached).sum()), first_pixel=int(firsts[i]),
                         box_xywh=(int(us.min()), int(vs.min()), int(us.max() - us.min()), int(vs.max() - vs.min())),
                         z_lo=np.float32(z[m].min()), z_hi=np.float32(z[m].max())))
    counts = (len(ranked), int(valid.sum()), len(firsts))
    stats = dict(n_kept=int(kept.sum()), n_eligible=int(eligible.sum()), n_smooth=int(smooth.sum()), n_attached=int(attached.sum()))
    return labels, info, counts, stats


def _check(depth_abs, depth_quad, normal_cos, curvature_threshold, min_size, max_size, max_segments, flags):
    ok = (np.isfinite(depth_abs) and depth_abs >= 0 and np.isfinite(depth_quad) and depth_quad >= 0 and np.isfinite(normal_cos)
          and -1 <= normal_cos <= 1 and curvature_threshold >= 0 and min_size >= 1 and max_size >= 0
          and 1 <= max_segments <= MAX_SEGMENTS and not (flags & ~(EIGHT | UNORIENTED)))
    if not ok:
        raise ValueError("a segment parameter is outside its range")


def segments(depth, *, depth_scale=0.001, z_min=0.0, z_max=0.0, normals=None, depth_abs=0.005, depth_quad=0.0, normal_cos=0.9659258,
             curvature_threshold=0.03, min_size=100, max_size=0, max_segments=64, flags=0):
    """(labels int32 image, info: one dict per segment, counts (segments, valid, all), stats: the four pixel counts).
    normals: None or (rows (n_kept, 6), curvature (n_kept,)) as ppf_cloud_from_depth_normals gives them"""
    _check(depth_abs, depth_quad, normal_cos, curvature_threshold, min_size, max_size, max_segments, flags)
    z, kept, eligible, smooth, nrm = classify(depth, normals, depth_scale, z_min, z_max, curvature_threshold)
    rows, cols = z.shape
    Z = z.astype(np.float64)
    A, Q, C = _f32(depth_abs), _f32(depth_quad), _f32(normal_cos)
    n64 = None if nrm is None else nrm.astype(np.float64)

    def shifted(a, dv, du):
        """(a at p, a at p + (dv, du)) over the pixels p whose neighbour is inside the image, and p's (v, u) slices"""
        v0, v1 = max(0, -dv), rows - max(0, dv)
        u0, u1 = max(0, -du), cols - max(0, du)
        return a[v0:v1, u0:u1], a[v0 + dv:v1 + dv, u0 + du:u1 + du], (slice(v0, v1), slice(u0, u1))

    def link(dv, du):
        """step and agree between p and p + (dv, du), as an image over p (False where the neighbour is outside)"""
        out = np.zeros(z.shape, bool)
        zp, zq, at = shifted(Z, dv, du)
        with np.errstate(all="ignore"):
            ok = np.abs(zq - zp) <= A + Q * (zp * zq)
            if n64 is not None:
                a, b, _ = shifted(n64, dv, du)
                dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
                if flags & UNORIENTED:
                    dot = np.abs(dot)
                ok &= dot >= C
        out[at] = ok
        return out

    parent = np.arange(rows * cols)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for dv, du in (FORWARD8 if flags & EIGHT else FORWARD4):
        sp, sq, at = shifted(smooth, dv, du)
        m = np.zeros(z.shape, bool)
        m[at] = sp & sq
        m &= link(dv, du)
        for p in np.flatnonzero(m):
            a, b = find(int(p)), find(int(p) + dv * cols + du)
            if a != b:
                parent[max(a, b)] = min(a, b)
    comp = np.full(rows * cols, -1, np.int64)
    for p in np.flatnonzero(smooth):
        comp[p] = find(int(p))
    comp = comp.reshape(z.shape)
    # border pixels: the linkable smooth neighbour nearest in Z, neighbours visited in ascending pixel index
    border = eligible & ~smooth
    best = np.full(z.shape, np.inf)
    choice = np.full(z.shape, -1, np.int64)
    for dv, du in (AROUND8 if flags & EIGHT else AROUND4):
        _, sq, at = shifted(smooth, dv, du)
        zp, zq, _ = shifted(Z, dv, du)
        _, cq, _ = shifted(comp, dv, du)
        cand = np.zeros(z.shape, bool)
        cand[at] = sq
        cand &= border & link(dv, du)
        d = np.full(z.shape, np.inf)
        with np.errstate(all="ignore"):
            d[at] = np.abs(zq - zp)
        better = cand & ((choice < 0) | (d < best))
        full_c = np.full(z.shape, -1, np.int64)
        full_c[at] = cq
        best[better] = d[better]
        choice[better] = full_c[better]
    attached = border & (choice >= 0)
    comp[attached] = choice[attached]
    return _finish(z, kept, eligible, smooth, comp, attached, min_size, max_size, max_segments)


def segments_bfs(depth, *, depth_scale=0.001, z_min=0.0, z_max=0.0, normals=None, depth_abs=0.005, depth_quad=0.0, normal_cos=0.9659258,
                 curvature_threshold=0.03, min_size=100, max_size=0, max_segments=64, flags=0):
    """the same, pixel by pixel: Python doubles, a breadth-first search per component"""
    _check(depth_abs, depth_quad, normal_cos, curvature_threshold, min_size, max_size, max_segments, flags)
    z, kept, eligible, smooth, nrm = classify(depth, normals, depth_scale, z_min, z_max, curvature_threshold)
    rows, cols = z.shape
    A, Q, C = float(np.float32(depth_abs)), float(np.float32(depth_quad)), float(np.float32(normal_cos))
    around = AROUND8 if flags & EIGHT else AROUND4

    def linked(pv, pu, qv, qu):
        zp, zq = float(z[pv, pu]), float(z[qv, qu])
        if not abs(zq - zp) <= A + Q * (zp * zq):
            return False
        if nrm is None:
            return True
        a, b = [float(x) for x in nrm[pv, pu]], [float(x) for x in nrm[qv, qu]]
        dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
        return (abs(dot) if flags & UNORIENTED else dot) >= C

    comp = np.full(z.shape, -1, np.int64)
    for v in range(rows):
        for u in range(cols):
            if not smooth[v, u] or comp[v, u] >= 0:
                continue
            first = v * cols + u                  # row-major scan: the first pixel met is the component's smallest
            comp[v, u] = first
            todo = deque([(v, u)])
            while todo:
                pv, pu = todo.popleft()
                for dv, du in around:
                    qv, qu = pv + dv, pu + du
                    if 0 <= qv < rows and 0 <= qu < cols and smooth[qv, qu] and comp[qv, qu] < 0 and linked(pv, pu, qv, qu):
                        comp[qv, qu] = first
                        todo.append((qv, qu))
    attached = np.zeros(z.shape, bool)
    joins = []
    for v, u in zip(*np.nonzero(eligible & ~smooth)):
        best = None
        for dv, du in around:
            qv, qu = v + dv, u + du
            if 0 <= qv < rows and 0 <= qu < cols and smooth[qv, qu] and linked(v, u, qv, qu):
                d = abs(float(z[qv, qu]) - float(z[v, u]))
                if best is None or d < best[0]:
                    best = (d, comp[qv, qu])
        if best is not None:
            joins.append((v, u, best[1]))
    for v, u, c in joins:
        comp[v, u] = c
        attached[v, u] = True
    return _finish(z, kept, eligible, smooth, comp, attached, min_size, max_size, max_segments)


def same(a, b):
    """two results agree in every output"""
    return (a[0].tobytes() == b[0].tobytes() and a[2] == b[2] and a[3] == b[3] and len(a[1]) == len(b[1])
            and all(x == y for x, y in zip(a[1], b[1])))
