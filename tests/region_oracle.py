"""The CPU restatement of ppf_prep_regions in numpy / scipy, which the device is held to byte for byte.

A row is eligible iff x, y, z, nx, ny, nz are finite; an eligible row is smooth iff curvature <= curvature_threshold (float32,
so a NaN curvature is not smooth), else a border row.  near(a, b) iff ((dx*dx + dy*dy) + dz*dz) <= (double)tol * (double)tol,
agree(a, b) iff ((anx*bnx + any*bny) + anz*bnz) >= (double)normal_cos (its absolute value with PPF_REGION_UNORIENTED), every
operation in fp64 as written.  Two smooth rows are linked iff near and agree; a component is a connected component of the links
over the smooth rows, named by its smallest smooth row.  A border row joins the component of the smooth row of the smallest
(squared distance, row index) among those it is near to and agrees with, or none.  From n_rows on (smooth plus attached rows)
everything is cluster_oracle's rule.  Candidate pairs come from a k-d tree with a radius a millionth larger than the tolerance
and are then filtered by the exact predicates, so the tree's own arithmetic decides nothing."""
import numpy as np

import cluster_oracle as CL

INFO = CL.INFO
UNORIENTED = 1
DEFAULTS = dict(tolerance=0.01, normal_cos=0.9659258, curvature_threshold=0.03, min_size=100, max_size=0, max_regions=64, flags=0)


def params(p=None):
    out = dict(DEFAULTS)
    out.update(p or {})
    return out


def dist2(a, b):
    """the squared distance of near(), rows of a against rows of b (fp64 arrays (..., 3) of values that were float32)"""
    d = a - b
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def agree(a, b, normal_cos, flags=0):
    """the normals' predicate, rows of a against rows of b (fp64 arrays (..., 3))"""
    dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    return (np.abs(dot) if flags & UNORIENTED else dot) >= float(np.float32(normal_cos))


def kinds(rows, curv, curvature_threshold):
    """(smooth, border) masks of (n, 6) float32 rows"""
    eligible = np.isfinite(rows).all(axis=1)
    with np.errstate(invalid="ignore"):
        smooth = eligible & (np.asarray(curv, np.float32) <= np.float32(curvature_threshold))
    return smooth, eligible & ~smooth


def _assemble(n, smooth, border, links, cand):
    """links: (m, 2) linked smooth pairs; cand: the arrays (border row, smooth row, squared distance) of the attachable pairs.
    Returns (per row the component's smallest smooth row or -1, the number of attached border rows)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    out = np.full(n, -1, np.int64)
    idx = np.flatnonzero(smooth)
    if idx.size:
        pos = np.full(n, -1, np.int64)
        pos[idx] = np.arange(idx.size)
        graph = coo_matrix((np.ones(links.shape[0], np.int8), (pos[links[:, 0]], pos[links[:, 1]])), shape=(idx.size, idx.size))
        _, comp = connected_components(graph, directed=False)
        first = np.full(comp.max() + 1, n, np.int64)
        np.minimum.at(first, comp, idx)
        out[idx] = first[comp]
    attached = 0
    b, a, d2 = cand
    if b.size:
        assert (d2 >= 0).all()                       # non-negative: the bit pattern orders it as the value does
        order = np.lexsort((a, np.ascontiguousarray(d2).view(np.uint64), b))
        b, a = b[order], a[order]
        lead = np.concatenate([[True], b[1:] != b[:-1]])
        out[b[lead]] = out[a[lead]]
        attached = int(lead.sum())
    return out, attached


def components(rows, curv, p=None):
    """(labels per row: the component's smallest smooth row, -1 for a row of no region; attached border rows)"""
    from scipy.spatial import cKDTree
    p = params(p)
    rows = np.asarray(rows, dtype=np.float32)
    n = rows.shape[0]
    smooth, border = kinds(rows, curv, p["curvature_threshold"])
    links, cand = np.zeros((0, 2), np.int64), (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    si, bi = np.flatnonzero(smooth), np.flatnonzero(border)
    if si.size:
        tol = float(np.float32(p["tolerance"]))
        reach = tol * (1 + 1e-6)
        pts, nrm = rows[:, :3].astype(np.float64), rows[:, 3:].astype(np.float64)
        tree = cKDTree(pts[si])

        def exact(a, b):
            d2 = dist2(pts[a], pts[b])
            ok = (d2 <= tol * tol) & agree(nrm[a], nrm[b], p["normal_cos"], p["flags"])
            return a[ok], b[ok], d2[ok]
        pairs = tree.query_pairs(reach, output_type="ndarray")
        a, b, _ = exact(si[pairs[:, 0]], si[pairs[:, 1]])
        links = np.stack([a, b], axis=1)
        if bi.size:                                   # border rows against smooth rows only: border rows link nothing
            near = cKDTree(pts[bi]).sparse_distance_matrix(tree, reach, output_type="coo_matrix")
            cand = exact(bi[near.row], si[near.col])
    return _assemble(n, smooth, border, links, cand)


def brute_components(rows, curv, p=None):
    """components() by the O(n^2) predicates: for small clouds, independent of the k-d tree"""
    p = params(p)
    rows = np.asarray(rows, dtype=np.float32)
    n = rows.shape[0]
    smooth, border = kinds(rows, curv, p["curvature_threshold"])
    pts, nrm = rows[:, :3].astype(np.float64), rows[:, 3:].astype(np.float64)
    tol = float(np.float32(p["tolerance"]))
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = dist2(pts[:, None, :], pts[None, :, :])
        ok = (d2 <= tol * tol) & agree(nrm[:, None, :], nrm[None, :, :], p["normal_cos"], p["flags"])
    adj = ok & smooth[:, None] & smooth[None, :]
    out = np.where(smooth, np.arange(n), n).astype(np.int64)
    while True:   # every smooth row takes the smallest label among its neighbours until nothing changes
        new = np.where(smooth, np.minimum(out, np.where(adj, out[None, :], n).min(axis=1, initial=n)), n)
        if (new == out).all():
            break
        out = new
    out[~smooth] = -1
    attached = 0
    for b in np.flatnonzero(border):
        can = ok[b] & smooth
        if can.any():
            out[b] = out[np.argmin(np.where(can, d2[b], np.inf))]   # the first minimum: the smaller row index
            attached += 1
    return out, attached


def regions(rows, p=None, curv=None, intr=None, image_size=None, brute=False):
    """rows: (n, 6) float32.  Returns (list of (region rows (m, 6), curvature (m,)), info (max_regions,) records, counts (4,) =
    regions output, valid components, all components, border rows attached, labels (n,) int32)"""
    p = params(p)
    full = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 6)
    n = full.shape[0]
    curv = np.zeros(n, np.float32) if curv is None else np.asarray(curv, dtype=np.float32)
    mc = int(p["max_regions"])
    info = np.zeros(mc, INFO)
    labels = np.full(n, -1, np.int32)
    comp, attached = (brute_components if brute else components)(full, curv, p)
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
            info[r]["lo"][a], info[r]["hi"][a] = CL._fmin(part[:, a]), CL._fmax(part[:, a])
        info[r]["box_xywh"] = CL.boxes_of(part, intr, image_size)
        found.append((part, curv[member]))
    return found, info, np.array([len(order), int(ok.sum()), first.size, attached], np.int32), labels
