"""A numpy restatement of ppf_depth_volume_mesh (the comment above the entry in include/ppf_hip.h): the zero
surface of a depth_volume_oracle.Volume as a triangle mesh by marching tetrahedra, six per cube.  The table is generated here
from the rule's two sentences; a vertex exists because a triangle names it; positions and normals are EXTRACT's fp64
arithmetic (depth_volume_oracle.gradients), in the stated order.  Also here: the random volumes the tests write into a device
volume, and the edge bookkeeping the manifold checks use."""
import functools

import numpy as np

import depth_volume_oracle as O

F32, F64 = np.float32, np.float64
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
EDGE_NAMES = ("x", "y", "xy", "z", "xz", "yz", "xyz")
N_LAUNCHES, N_HOST_SYNCS = 14, 2


def corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], F64)


@functools.lru_cache(maxsize=None)
def table():
    """table[tet][case]: a tuple of 0, 1 or 2 triangles, each three edges (ca, cb) of cube corners with the bits of ca inside
    those of cb.  Bit n of `case` is set when corner t_n of the tetrahedron is positive."""
    out = []
    for tet in TETS:
        row = []
        for case in range(16):
            P = [tet[n] for n in range(4) if (case >> n) & 1]
            N = [tet[n] for n in range(4) if not (case >> n) & 1]
            if len(P) in (0, 4):
                tris = []
            elif len(P) == 1 or len(N) == 1:
                a = P[0] if len(P) == 1 else N[0]
                b = [c for c in tet if c != a]
                tris = [[(a, b[0]), (a, b[1]), (a, b[2])]]
            else:
                (a1, a2), (b1, b2) = N, P
                tris = [[(a1, b1), (a1, b2), (a2, b2)], [(a1, b1), (a2, b2), (a2, b1)]]
            fixed = []
            for tri in tris:
                mid = [(corner_xyz(ca) + corner_xyz(cb)) / 2.0 for ca, cb in tri]
                m = np.mean([corner_xyz(c) for c in P], axis=0) - np.mean([corner_xyz(c) for c in N], axis=0)
                s = float(np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), m))
                assert s != 0.0
                if s < 0:
                    tri = [tri[0], tri[2], tri[1]]
                fixed.append(tuple((min(e), max(e)) for e in tri))
            row.append(tuple(fixed))
        out.append(tuple(row))
    return tuple(out)


def random_volume(dims, seed, max_weight=3):
    """an O.Volume of `dims` with d uniform in (-1, 1), weights 0..3 (0: unobserved, which keeps d = 1), and a few saturated
    voxels (d = -1 or 1 with a weight)"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    vol = O.Volume(dims, 0.01, (-0.005 * (nx - 1) + 0.003, -0.005 * (ny - 1) - 0.002, 0.6), 0.025, max_weight=max_weight)
    d = rng.uniform(-1.0, 1.0, size=(nz, ny, nx)).astype(F32)
    d = np.where(np.abs(d) < 1, d, F32(0.5)).astype(F32)
    w = rng.choice(4, size=(nz, ny, nx), p=(0.08, 0.12, 0.4, 0.4)).astype(np.int32)   # few holes: cubes are active at weight 2 too
    sat = rng.random((nz, ny, nx)) < 0.03
    d = np.where(sat, np.where(rng.random((nz, ny, nx)) < 0.5, F32(1), F32(-1)), d).astype(F32)
    d = np.where(w == 0, F32(1), d).astype(F32)
    vol.d, vol.w = np.ascontiguousarray(d), np.ascontiguousarray(w)
    return vol


def volume_params(vol):
    """the keywords DepthVolume takes for the volume of an O.Volume"""
    return dict(dims=vol.dims, voxel=float(vol.voxel), origin=vol.origin, trunc=float(vol.trunc), max_weight=vol.max_weight)


def _shift(a, c):
    """the array of corner c of every cube: a[k + dz, j + dy, i + dx] for the cubes' corner-0 voxels"""
    nz, ny, nx = a.shape[:3]
    dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
    return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def cubes(vol, min_weight=1):
    """(active (nz-1, ny-1, nx-1) bool, positive: eight such arrays, one per corner); None when the volume has no cubes"""
    if min(vol.d.shape) < 2:
        return None
    d = vol.d.astype(F64)
    valid = (vol.w >= min_weight) & (np.abs(d) < 1)
    pos = d > 0
    active = np.ones(_shift(valid, 0).shape, bool)
    for c in range(8):
        active &= _shift(valid, c)
    return active, [_shift(pos, c) for c in range(8)]


def triangles_by_key(vol, min_weight=1):
    """(keys (M, 3) int64: owner's linear voxel index * 7 + edge type, in (cube, tet, triangle) order; cases (n, 2): the
    (tet, case) of every tetrahedron of an active cube; n_cells)"""
    cb = cubes(vol, min_weight)
    if cb is None:
        return np.zeros((0, 3), np.int64), np.zeros((0, 2), np.int64), 0
    active, pos = cb
    nz, ny, nx = vol.d.shape
    lin = np.arange(nz * ny * nx, dtype=np.int64).reshape(nz, ny, nx)
    lin0 = _shift(lin, 0)[active]
    off = [(c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny for c in range(8)]
    T = table()
    order, keys, seen = [], [], []
    for ti, tet in enumerate(TETS):
        case = np.zeros(lin0.shape, np.int64)
        for n in range(4):
            case |= pos[tet[n]][active].astype(np.int64) << n
        seen.append(np.stack([np.full(case.shape, ti, np.int64), case], -1))
        for cs in range(1, 15):
            sel = lin0[case == cs]
            for tri_i, tri in enumerate(T[ti][cs]):
                order.append(np.stack([sel, np.full(sel.shape, ti, np.int64), np.full(sel.shape, tri_i, np.int64)], -1))
                keys.append(np.stack([(sel + off[ca]) * 7 + ((ca ^ cb_) - 1) for ca, cb_ in tri], -1))
    order, keys = np.concatenate(order), np.concatenate(keys)
    perm = np.lexsort((order[:, 2], order[:, 1], order[:, 0]))
    return keys[perm], np.concatenate(seen), int(active.sum())


def vertex_rows(vol, vkeys, min_weight=1):
    """rows x y z nx ny nz (float32) of the vertices with the sorted keys vkeys, and how many have no normal"""
    nz, ny, nx = vol.d.shape
    owner, e = vkeys // 7, vkeys % 7
    D = e + 1
    i, j, k = owner % nx, (owner // nx) % ny, owner // (nx * ny)
    i1, j1, k1 = i + (D & 1), j + ((D >> 1) & 1), k + ((D >> 2) & 1)
    d = vol.d.astype(F64)
    gok, g = O.gradients(vol, min_weight)
    c = vol.centres()
    with np.errstate(all="ignore"):
        d0, d1 = d[k, j, i], d[k1, j1, i1]
        t = d0 / (d0 - d1)
        m = t * vol.v64
        gg = [g[b][k, j, i] + t * (g[b][k1, j1, i1] - g[b][k, j, i]) for b in range(3)]
        ln = np.sqrt((gg[0] * gg[0] + gg[1] * gg[1]) + gg[2] * gg[2])
        ok = gok[k, j, i] & gok[k1, j1, i1] & (ln > 0)
        rows = np.zeros((len(vkeys), 6), F32)
        for b, idx in enumerate((i, j, k)):
            rows[:, b] = np.where((D >> b) & 1, c[b][idx] + m, c[b][idx]).astype(F32)
            rows[:, 3 + b] = np.where(ok, gg[b] / ln, 0.0).astype(F32)
    return rows, int((~ok).sum())


def mesh(vol, min_weight=1):
    """(vertices (N, 6) float32 in (owner's linear voxel index, type) order, triangles (M, 3) int32 in (cube, tet, triangle)
    order, stats)"""
    tkeys, _, n_cells = triangles_by_key(vol, min_weight)
    vkeys = np.unique(tkeys)
    tris = np.searchsorted(vkeys, tkeys).astype(np.int32).reshape(-1, 3)
    rows, n_no = vertex_rows(vol, vkeys, min_weight)
    stats = dict(n_cells=n_cells, n_vertices=len(vkeys), n_triangles=len(tris), n_no_normal=n_no, n_launches=N_LAUNCHES,
                 n_host_syncs=N_HOST_SYNCS)
    return rows, np.ascontiguousarray(tris), stats


def vertex_keys_by_rule(vol, min_weight=1):
    """the sorted keys of the edges whose two end voxels differ in `positive` and that at least one active cube contains"""
    cb = cubes(vol, min_weight)
    if cb is None:
        return np.zeros(0, np.int64)
    active, _ = cb
    nz, ny, nx = vol.d.shape
    pos = vol.d.astype(F64) > 0
    lin = np.arange(nz * ny * nx, dtype=np.int64).reshape(nz, ny, nx)
    keys = []
    for e in range(7):
        D = e + 1
        for off in range(8):
            if off & D:
                continue
            differ = _shift(pos, off) != _shift(pos, off | D)
            keys.append(_shift(lin, off)[active & differ] * 7 + e)
    return np.unique(np.concatenate(keys))


def edge_counts(tris):
    """(undirected: {(a, b): uses}, directed: {(a, b): uses}) of a triangle list"""
    und, dr = {}, {}
    for t in np.asarray(tris).reshape(-1, 3).tolist():
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            dr[a, b] = dr.get((a, b), 0) + 1
            key = (min(a, b), max(a, b))
            und[key] = und.get(key, 0) + 1
    return und, dr


def face_normals(vertices, tris):
    """(unit face normals (M, 3) float64, centroids (M, 3), doubled areas (M))"""
    p = np.asarray(vertices)[:, :3].astype(F64)[np.asarray(tris).reshape(-1, 3)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    a2 = np.linalg.norm(n, axis=1)
    with np.errstate(all="ignore"):
        return n / a2[:, None], p.mean(axis=1), a2


def fnv1a(data: bytes) -> int:
    h = 14695981039346656037
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h
