"""COMPONENTS (include/ppf_hip.h) restated in numpy, sharing nothing with the engine: a plain union-find by label
propagation, the area formula as written, np.unique on the edge pairs.  ``components`` is vectorised; ``components_loops`` is
the same specification in plain Python loops, for small meshes.  Both return a dict:

  labels (nv int32)   info (C records, rank order, every component)   out_vertices / out_triangles
  n_components n_kept n_unreferenced n_bad_area n_vertices_out n_triangles_out

Also here: the meshes that the CPU test and the device test share."""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
INT32_MAX = 2 ** 31 - 1
N_LAUNCHES, N_LAUNCHES_MEASURE, N_HOST_SYNCS = 82, 80, 2
# ppf_mesh_component_info
INFO = np.dtype([("n_vertices", "<i4"), ("n_triangles", "<i4"), ("n_degenerate", "<i4"), ("n_edges", "<i4"), ("n_boundary_edges", "<i4"),
                 ("n_nonmanifold_edges", "<i4"), ("first_vertex", "<i4"), ("kept", "<i4"), ("area", "<f8"), ("lo", "<f4", 3), ("hi", "<f4", 3),
                 ("reserved", "<i4", 2)])
assert INFO.itemsize == 72
COUNTS = ("n_components", "n_kept", "n_unreferenced", "n_bad_area", "n_vertices_out", "n_triangles_out")
TWO40, TWO63 = 2.0 ** 40, 2.0 ** 63


def as_mesh(vertices, triangles):
    v = np.ascontiguousarray(vertices, F32)
    if v.ndim != 2 or v.shape[1] == 3:
        v = np.concatenate([v.reshape(-1, 3), np.zeros((v.size // 3, 3), F32)], axis=1)
    return np.ascontiguousarray(v[:, :6]), np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)


def roots_by_propagation(nv, t):
    """lab[v]: the smallest vertex index of v's class, by hooking every class under the smallest class a triangle joins it to and
    jumping pointers until nothing moves"""
    lab = np.arange(nv, dtype=np.int64)
    if len(t) == 0:
        return lab
    while True:
        l = lab[t]
        new = lab.copy()
        np.minimum.at(new, l.reshape(-1), np.repeat(l.min(axis=1), 3))
        while True:
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, lab):
            return lab
        lab = new


def areas_q(v, t):
    """(q uint64 per triangle, bad per triangle)"""
    P = v[:, :3].astype(F64)
    a, b = P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]]
    with np.errstate(all="ignore"):
        cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        A = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
        s = A * TWO40
        bad = ~np.isfinite(A) | ~(s < TWO63)
    return np.floor(np.where(bad, 0.0, s)).astype(np.uint64), bad


def signed_zero_order(x):
    """float64 copies in which -0 lies strictly below +0, and the way back"""
    x = x.astype(F64)
    return np.where((x == 0) & np.signbit(x), -5e-324, x)


def finish(v, t, first, per, min_triangles, min_area, rank_lo, rank_hi, lab, referenced, n_bad):
    """from the per-component sums (in first_vertex order) to the result: rank, kept, labels, the output mesh"""
    nv, C = len(v), len(first)
    order = np.lexsort((first, ~per["area_q"])) if C else np.zeros(0, np.int64)
    info = np.zeros(C, INFO)
    for name in ("n_vertices", "n_triangles", "n_degenerate", "n_edges", "n_boundary_edges", "n_nonmanifold_edges"):
        info[name] = per[name][order]
    info["first_vertex"] = first[order]
    info["area"] = per["area_q"][order].astype(F64) * 2.0 ** -40
    info["lo"], info["hi"] = per["lo"][order], per["hi"][order]
    rank = np.arange(C)
    info["kept"] = (rank >= rank_lo) & (rank < rank_hi) & (info["n_triangles"] >= min_triangles) & (info["area"] >= float(F32(min_area)))
    rank_of_first = np.full(nv + 1, -1, np.int64)
    rank_of_first[first[order]] = rank
    labels = np.where(referenced, rank_of_first[lab], -1).astype(np.int32)
    vkeep = np.zeros(nv, bool)
    vkeep[referenced] = info["kept"][labels[referenced]].astype(bool)
    new_index = np.cumsum(vkeep) - 1
    tkeep = vkeep[t[:, 0]] if len(t) else np.zeros(0, bool)
    out_t = new_index[t[tkeep]].astype(np.int32).reshape(-1, 3)
    out_v = v[vkeep]
    return dict(labels=labels, info=info, out_vertices=np.ascontiguousarray(out_v), out_triangles=np.ascontiguousarray(out_t),
                n_components=C, n_kept=int(info["kept"].sum()), n_unreferenced=int((~referenced).sum()), n_bad_area=int(n_bad),
                n_vertices_out=len(out_v), n_triangles_out=len(out_t))


def components(vertices, triangles, min_triangles=1, min_area=0.0, rank_lo=0, rank_hi=INT32_MAX):
    return select(measure(vertices, triangles), min_triangles, min_area, rank_lo, rank_hi)


def select(measured, min_triangles=1, min_area=0.0, rank_lo=0, rank_hi=INT32_MAX):
    """the result for one set of parameters from what ``measure`` found, which does not depend on them"""
    v, t, first, per, lab, referenced, n_bad = measured
    return finish(v, t, first, per, min_triangles, min_area, rank_lo, rank_hi, lab, referenced, n_bad)


def measure(vertices, triangles):
    v, t = as_mesh(vertices, triangles)
    nv = len(v)
    t64 = t.astype(np.int64)
    referenced = np.zeros(nv, bool)
    referenced[t64.reshape(-1)] = True
    lab = roots_by_propagation(nv, t64)
    first = np.flatnonzero(referenced & (lab == np.arange(nv)))
    cid = np.full(nv, -1, np.int64)
    cid[first] = np.arange(len(first))
    C = len(first)
    tc = cid[lab[t64[:, 0]]] if len(t) else np.zeros(0, np.int64)
    vc = cid[lab]
    deg = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    q, bad = areas_q(v, t64)
    per = dict(n_vertices=np.bincount(vc[referenced], minlength=C), n_triangles=np.bincount(tc, minlength=C),
               n_degenerate=np.bincount(tc[deg], minlength=C), area_q=np.zeros(C, np.uint64))
    np.add.at(per["area_q"], tc, q)
    # edges of the non-degenerate triangles
    g = t64[~deg]
    pairs = np.concatenate([g[:, [0, 1]], g[:, [1, 2]], g[:, [2, 0]]]) if len(g) else np.zeros((0, 2), np.int64)
    key = pairs.min(axis=1) << 32 | pairs.max(axis=1)
    uk, mult = np.unique(key, return_counts=True)
    ec = cid[lab[uk >> 32]]
    per["n_edges"] = np.bincount(ec, minlength=C)
    per["n_boundary_edges"] = np.bincount(ec[mult == 1], minlength=C)
    per["n_nonmanifold_edges"] = np.bincount(ec[mult > 2], minlength=C)
    # bounds, -0 below +0
    z = signed_zero_order(v[:, :3])
    lo, hi = np.full((C, 3), np.inf), np.full((C, 3), -np.inf)
    np.minimum.at(lo, vc[referenced], z[referenced])
    np.maximum.at(hi, vc[referenced], z[referenced])
    back = lambda x: np.where(x == -5e-324, -0.0, x).astype(F32)
    per["lo"], per["hi"] = back(lo), back(hi)
    return v, t, first, per, lab, referenced, bad.sum()


def components_loops(vertices, triangles, min_triangles=1, min_area=0.0, rank_lo=0, rank_hi=INT32_MAX):
    """the specification in plain Python: a union-find with path compression, scalar fp64 arithmetic, dictionaries"""
    v, t = as_mesh(vertices, triangles)
    nv = len(v)
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    referenced = np.zeros(nv, bool)
    for i0, i1, i2 in t.tolist():
        referenced[[i0, i1, i2]] = True
        unite(i0, i1)
        unite(i0, i2)
    lab = np.array([find(x) for x in range(nv)], np.int64).reshape(nv)
    first = np.array(sorted({int(lab[x]) for x in range(nv) if referenced[x]}), np.int64)
    cid = {int(f): n for n, f in enumerate(first)}
    C = len(first)
    per = {k: np.zeros(C, np.int64) for k in ("n_vertices", "n_triangles", "n_degenerate", "n_edges", "n_boundary_edges", "n_nonmanifold_edges")}
    area_q = [0] * C
    lo, hi = [[None] * 3 for _ in range(C)], [[None] * 3 for _ in range(C)]
    below = lambda a, b: a < b or (a == b and math.copysign(1.0, a) < math.copysign(1.0, b))
    for x in range(nv):
        if referenced[x]:
            c = cid[int(lab[x])]
            per["n_vertices"][c] += 1
            for ax in range(3):
                val = float(v[x, ax])
                if lo[c][ax] is None or below(val, lo[c][ax]):
                    lo[c][ax] = val
                if hi[c][ax] is None or below(hi[c][ax], val):
                    hi[c][ax] = val
    edges, n_bad = {}, 0
    P = v[:, :3].astype(F64).tolist()
    for i0, i1, i2 in t.tolist():
        c = cid[int(lab[i0])]
        per["n_triangles"][c] += 1
        a = [P[i1][ax] - P[i0][ax] for ax in range(3)]
        b = [P[i2][ax] - P[i0][ax] for ax in range(3)]
        cx, cy, cz = a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]
        try:
            A = 0.5 * math.sqrt((cx * cx + cy * cy) + cz * cz)
        except (OverflowError, ValueError):
            A = math.inf
        if not math.isfinite(A) or not (A * TWO40 < TWO63):
            n_bad += 1
        else:
            area_q[c] = (area_q[c] + int(math.floor(A * TWO40))) % (1 << 64)
        if len({i0, i1, i2}) < 3:
            per["n_degenerate"][c] += 1
            continue
        for e in ((i0, i1), (i1, i2), (i2, i0)):
            e = (min(e), max(e))
            edges[e] = edges.get(e, 0) + 1
    for (a, _), mult in edges.items():
        c = cid[int(lab[a])]
        per["n_edges"][c] += 1
        per["n_boundary_edges"][c] += mult == 1
        per["n_nonmanifold_edges"][c] += mult > 2
    per["area_q"] = np.array(area_q, np.uint64).reshape(C)
    per["lo"], per["hi"] = np.array(lo, F32).reshape(C, 3), np.array(hi, F32).reshape(C, 3)
    return finish(v, t, first, per, min_triangles, min_area, rank_lo, rank_hi, lab, referenced, n_bad)


def euler(rec):
    return int(rec["n_vertices"]) - int(rec["n_edges"]) + int(rec["n_triangles"])


def same(a, b):
    """the names under which two results differ"""
    diff = [k for k in COUNTS if a[k] != b[k]]
    diff += [k for k in ("labels", "info", "out_vertices", "out_triangles")
             if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    return diff


# ---- meshes ----------------------------------------------------------------------------------------------------------
def grid(n, m, origin=(0.0, 0.0, 0.0), step=0.25):
    """an n x m grid of squares, two triangles each, on exactly representable coordinates"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(m + 1), indexing="ij")
    v = np.stack([origin[0] + step * i, origin[1] + step * j, np.full(i.shape, origin[2])], -1).reshape(-1, 3).astype(F32)
    idx = lambda a, b: a * (m + 1) + b
    t = [[idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)] for a in range(n) for b in range(m)]
    t += [[idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)] for a in range(n) for b in range(m)]
    return v, np.array(t, np.int32)


def join(*meshes):
    vs, ts, base = [], [], 0
    for v, t in meshes:
        v, t = as_mesh(v, t)
        vs.append(v)
        ts.append(t + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(ts).astype(np.int32)


TRI_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)


def hand_made():
    """name -> (vertices, triangles): meshes whose answers are known"""
    tet_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    two_pieces = join((TRI_V, [[0, 1, 2]]), (TRI_V + F32(4), [[0, 1, 2]]))
    huge = TRI_V.copy()
    huge[1, 0] = 1e30
    huge[2, 1] = 1e30
    piece = grid(2, 1)
    return {
        "one triangle": (TRI_V, np.array([[0, 1, 2]], np.int32)),
        "shared edge": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], F32), np.array([[0, 1, 2], [1, 3, 2]], np.int32)),
        "shared vertex": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], F32), np.array([[0, 1, 2], [0, 3, 4]], np.int32)),
        "tetrahedron": (tet_v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)),
        "three on an edge": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], F32),
                             np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int32)),
        "degenerate bridge": (two_pieces[0], np.concatenate([two_pieces[1], [[2, 2, 3]]]).astype(np.int32)),
        "unreferenced vertex": (np.concatenate([[[9, 9, 9]], TRI_V, [[7, 7, 7]]]).astype(F32), np.array([[1, 2, 3]], np.int32)),
        "huge coordinate": join((huge, [[0, 1, 2]]), (TRI_V - F32(3), [[0, 1, 2]])),
        "congruent pieces": join(piece, (piece[0] + F32(8), piece[1]), (TRI_V - F32(5), [[0, 1, 2]])),
        "signed zeros": (np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, 1.0], [1.0, -0.0, 0.0]], F32), np.array([[0, 1, 2]], np.int32)),
        "empty": (np.zeros((0, 6), F32), np.zeros((0, 3), np.int32)),
        "vertices only": (TRI_V, np.zeros((0, 3), np.int32)),
    }


def random_mesh(nv, nt, seed, normals=True):
    """nt random triangles over nv vertices: some degenerate, some repeated; the density nt / nv decides how many components"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (nv, 6 if normals else 3)).astype(F32)
    t = rng.integers(0, nv, (nt, 3)).astype(np.int32)
    if nt > 4:
        t[nt // 2] = t[nt // 3]             # the same triangle twice
        t[nt // 4, 1] = t[nt // 4, 0]       # a degenerate one
    return v, t


def strip(n_triangles, seed):
    """a strip of triangles k, k + 1, k + 2 whose vertex numbering is a seeded permutation: one component through long chains"""
    rng = np.random.default_rng(seed)
    nv = n_triangles + 2
    perm = rng.permutation(nv).astype(np.int32)
    k = np.arange(n_triangles)
    t = perm[np.stack([k, k + 1, k + 2], 1)]
    pos = np.zeros((nv, 3), F32)
    pos[perm, 0] = (np.arange(nv) // 2 * 0.25).astype(F32)
    pos[perm, 1] = (np.arange(nv) % 2).astype(F32)
    return pos, t.astype(np.int32)


def isolated(n):
    """n triangles that share nothing; their sizes differ so that the ranks are not the input order"""
    rng = np.random.default_rng(n)
    scale = rng.integers(1, 64, n).astype(F32) * F32(0.125)
    v = (TRI_V[None] * scale[:, None, None]).reshape(-1, 3)
    v[:, 2] = np.repeat(np.arange(n), 3).astype(F32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def fan(n):
    """n triangles around vertex 0"""
    ang = np.arange(n + 1) * (2 * np.pi / (n + 1))
    v = np.concatenate([[[0, 0, 0]], np.stack([np.cos(ang), np.sin(ang), np.zeros(n + 1)], 1)]).astype(F32)
    k = np.arange(1, n + 1)
    return v, np.stack([np.zeros(n, np.int64), k, k + 1], 1).astype(np.int32)


def sized(nv):
    """a mesh of exactly nv vertices: a strip over the first nv - 1 (permuted) and one unreferenced vertex, around wave and
    workgroup edges"""
    v, t = strip(nv - 3, nv)
    return np.concatenate([v, [[5, 5, 5]]]).astype(F32), t


# ---- the project's scenes, through the numpy oracles of the volume and its mesh ----------------------------------------
@functools.lru_cache(maxsize=None)
def scene_volume(which):
    """the oracle volume of "sphere" (the fused sphere of §30 / §32) or "scan" (render_scan's two objects), four views at 64^3"""
    import depth_volume_cases as VC
    import depth_volume_oracle as O
    vol = O.Volume(**VC.SPHERE_VOLUME)
    intr = O.cases.intrinsics()
    for T in VC.SPHERE_VIEWS:
        O.integrate(vol, VC.render_sphere(T) if which == "sphere" else VC.render_scan(T), intr, T)
    return vol


@functools.lru_cache(maxsize=None)
def scene_mesh(which):
    import volume_mesh_oracle as M
    if isinstance(which, tuple):
        v, t, _ = M.mesh(M.random_volume(*which), 1)
    else:
        v, t, _ = M.mesh(scene_volume(which), 1)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def scene_components(which):
    return components(*scene_mesh(which))
