"""The CPU restatement of ppf_prep_clusters in numpy / scipy, which the device is held to byte for byte.

A row is finite iff x, y, z are.  Finite rows a, b are linked iff ((dx*dx + dy*dy) + dz*dz) <= (double)tol * (double)tol, with
dx = (double)ax - (double)bx ..., every operation in fp64 as written.  Candidate pairs come from a k-d tree with a radius a
millionth larger than the tolerance and are then filtered by that exact predicate, so the tree's own arithmetic decides
nothing.  A component is a connected component of the links; valid iff min_size <= n_rows and (max_size == 0 or n_rows <=
max_size); the valid ones ranked by n_rows descending, then first_row ascending; the first max_clusters are the clusters."""
import numpy as np

INFO = np.dtype([("n_rows", "<i4"), ("first_row", "<i4"), ("lo", "<f4", 3), ("hi", "<f4", 3), ("box_xywh", "<i4", 4),
                 ("reserved", "<i4", 4)])
DEFAULTS = dict(tolerance=0.02, min_size=100, max_size=0, max_clusters=64)


def params(p=None):
    out = dict(DEFAULTS)
    out.update(p or {})
    return out


def linked(a, b, tolerance):
    """the predicate, rows of a against rows of b (fp64 arrays (..., 3) of values that were float32)"""
    tol = float(np.float32(tolerance))
    d = a - b
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return ((dx * dx + dy * dy) + dz * dz) <= tol * tol


def _ordered(v):
    """float32 -> the uint32 whose order is the floats' (-0.0 below +0.0), as the device reduces minima and maxima"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def _fmin(v):
    return v[np.argmin(_ordered(v))]


def _fmax(v):
    return v[np.argmax(_ordered(v))]


def components(xyz, tolerance):
    """(labels per row: the component's smallest row index, -1 for a non-finite row)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    xyz = np.asarray(xyz, dtype=np.float32)[:, :3]
    n = xyz.shape[0]
    fin = np.isfinite(xyz).all(axis=1)
    idx = np.flatnonzero(fin)
    out = np.full(n, -1, np.int64)
    if idx.size == 0:
        return out
    pts = xyz[idx].astype(np.float64)
    tol = float(np.float32(tolerance))
    pairs = cKDTree(pts).query_pairs(tol * (1 + 1e-6), output_type="ndarray")
    pairs = pairs[linked(pts[pairs[:, 0]], pts[pairs[:, 1]], tolerance)]
    m = idx.size
    graph = coo_matrix((np.ones(pairs.shape[0], np.int8), (pairs[:, 0], pairs[:, 1])), shape=(m, m))
    _, comp = connected_components(graph, directed=False)
    first = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(first, comp, idx)
    out[idx] = first[comp]
    return out


def boxes_of(rows, intr, image_size):
    """the image box {umin, vmin, umax - umin, vmax - vmin} of the rows with z > 0, clipped to the image; zero without one"""
    if intr is None:
        return np.zeros(4, np.int32)
    fx, fy, ppx, ppy = [float(v) for v in intr]
    h, w = image_size
    q = rows[rows[:, 2] > 0, :3].astype(np.float64)
    if q.shape[0] == 0:
        return np.zeros(4, np.int32)
    with np.errstate(over="ignore"):
        u = np.clip(np.floor(((q[:, 0] / q[:, 2]) * fx + ppx) + 0.5), 0, w - 1).astype(np.int64)
        v = np.clip(np.floor(((q[:, 1] / q[:, 2]) * fy + ppy) + 0.5), 0, h - 1).astype(np.int64)
    return np.array([u.min(), v.min(), u.max() - u.min(), v.max() - v.min()], np.int32)


def clusters(rows, p=None, curv=None, intr=None, image_size=None):
    """rows: (n, 3) or (n, 6) float32.  Returns (list of (cluster rows (m, 6), curvature (m,)), info (max_clusters,) records,
    counts (3,) = clusters output, valid components, all components, labels (n,) int32)"""
    p = params(p)
    src = np.asarray(rows, dtype=np.float32)
    n = src.shape[0]
    full = np.zeros((n, 6), np.float32)
    full[:, :src.shape[1]] = src
    curv = np.zeros(n, np.float32) if curv is None else np.asarray(curv, dtype=np.float32)
    mc = int(p["max_clusters"])
    info = np.zeros(mc, INFO)
    labels = np.full(n, -1, np.int32)
    comp = components(full, p["tolerance"])
    first, size = np.unique(comp[comp >= 0], return_counts=True)
    ok = (size >= p["min_size"]) & ((p["max_size"] == 0) | (size <= p["max_size"]))
    vfirst, vsize = first[ok], size[ok]
    order = np.lexsort((vfirst, -vsize))[:mc]
    found = []
    for r, k in enumerate(order):
        member = comp == vfirst[k]
        labels[member] = r
        part = full[member]
        info[r]["n_rows"], info[r]["first_row"] = vsize[k], vfirst[k]
        for a in range(3):
            info[r]["lo"][a], info[r]["hi"][a] = _fmin(part[:, a]), _fmax(part[:, a])
        info[r]["box_xywh"] = boxes_of(part, intr, image_size)
        found.append((part, curv[member]))
    return found, info, np.array([len(order), int(ok.sum()), first.size], np.int32), labels


def brute_components(xyz, tolerance):
    """components() by the O(n^2) predicate and a plain union of labels: for small clouds, independent of the k-d tree"""
    xyz = np.asarray(xyz, dtype=np.float32)[:, :3]
    n = xyz.shape[0]
    fin = np.isfinite(xyz).all(axis=1)
    pts = xyz.astype(np.float64)
    out = np.where(fin, np.arange(n), -1).astype(np.int64)
    with np.errstate(invalid="ignore"):
        adj = linked(pts[:, None, :], pts[None, :, :], tolerance) & fin[:, None] & fin[None, :]
    while True:   # every row takes the smallest label among its neighbours until nothing changes
        best = np.where(adj, out[None, :], n).min(axis=1, initial=n)
        new = np.where(fin, np.minimum(out, best), -1)
        if (new == out).all():
            return out
        out = new
