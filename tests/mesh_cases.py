"""The meshes of the ppf_cloud_from_mesh tests: vertices (N, 3 | vstride) float32 and triangles (M, 3) int32, wound outward
unless a case says otherwise."""
import numpy as np


def rotation():
    """the one fixed rotation of the rotated cases: 0.7 rad about (1, 2, 3) / sqrt(14)"""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)


def rotated(mesh, Rm=None, shift=(0.013, -0.021, 0.034)):
    V, T = mesh
    Rm = rotation() if Rm is None else Rm
    W = V.astype(np.float64).copy()
    W[:, :3] = V[:, :3].astype(np.float64) @ Rm.T + np.asarray(shift)
    if V.shape[1] >= 6:
        W[:, -3:] = V[:, -3:].astype(np.float64) @ Rm.T
    return W.astype(np.float32), T


def box(a=0.10, b=0.14, c=0.20):
    """8 vertices, 12 triangles, centred on the origin"""
    V = np.array([[x, y, z] for x in (-a / 2, a / 2) for y in (-b / 2, b / 2) for z in (-c / 2, c / 2)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # -x +x -y +y -z +z, outward
    T = []
    for q in quads:
        T += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return V, np.array(T, dtype=np.int32)


def box_in_box(a=0.10, b=0.14, c=0.20, inner=0.6):
    """the box with every other outer triangle's winding reversed, and a second box of `inner` of its size inside, wound
    inward: triangles 0..11 are the outer ones, 12..23 the inner ones"""
    Vo, To = box(a, b, c)
    Vi, Ti = box(a * inner, b * inner, c * inner)
    To = To.copy()
    To[1::2] = To[1::2, ::-1]
    return np.concatenate([Vo, Vi]), np.concatenate([To, Ti[:, ::-1] + 8]).astype(np.int32)


def torus(R=0.06, r=0.02, nu=48, nv=24, with_normals=False, vstride=None, normal_offset=None):
    """nu x nv vertices, 2 nu nv triangles; with_normals: the analytic vertex normals at normal_offset of vstride floats"""
    u = np.arange(nu) * (2 * np.pi / nu)
    v = np.arange(nv) * (2 * np.pi / nv)
    U, Vv = np.meshgrid(u, v, indexing="ij")
    P = np.stack([(R + r * np.cos(Vv)) * np.cos(U), (R + r * np.cos(Vv)) * np.sin(U), r * np.sin(Vv)], axis=-1).reshape(-1, 3)
    N = np.stack([np.cos(Vv) * np.cos(U), np.cos(Vv) * np.sin(U), np.sin(Vv)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = (i * nv + j).reshape(-1), (((i + 1) % nu) * nv + j).reshape(-1)
    c, d = (((i + 1) % nu) * nv + (j + 1) % nv).reshape(-1), (i * nv + (j + 1) % nv).reshape(-1)
    T = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]).astype(np.int32)
    if not with_normals:
        return P.astype(np.float32), T
    vstride = 6 if vstride is None else vstride
    normal_offset = 3 if normal_offset is None else normal_offset
    V = np.full((len(P), vstride), 7.0, dtype=np.float32)  # the other columns hold a value nothing may read as geometry
    V[:, :3], V[:, normal_offset:normal_offset + 3] = P, N
    return V, T


def sphere(n_lat, n_lon, radius=0.08):
    """a latitude-longitude sphere of 2 n_lon (n_lat - 1) triangles"""
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.arange(n_lon) * (2 * np.pi / n_lon)
    Tt, Pp = np.meshgrid(th, ph, indexing="ij")
    P = radius * np.stack([np.sin(Tt) * np.cos(Pp), np.sin(Tt) * np.sin(Pp), np.cos(Tt)], axis=-1).reshape(-1, 3)
    P = np.concatenate([P, [[0, 0, radius], [0, 0, -radius]]])
    top, bot = len(P) - 2, len(P) - 1
    i, j = np.meshgrid(np.arange(n_lat - 2), np.arange(n_lon), indexing="ij")
    a, b = (i * n_lon + j).reshape(-1), (i * n_lon + (j + 1) % n_lon).reshape(-1)
    c, d = ((i + 1) * n_lon + (j + 1) % n_lon).reshape(-1), ((i + 1) * n_lon + j).reshape(-1)
    jj = np.arange(n_lon)
    last = (n_lat - 2) * n_lon
    T = np.concatenate([np.stack([a, d, c], axis=1), np.stack([a, c, b], axis=1),
                        np.stack([np.full(n_lon, top), jj, (jj + 1) % n_lon], axis=1),
                        np.stack([np.full(n_lon, bot), last + (jj + 1) % n_lon, last + jj], axis=1)]).astype(np.int32)
    return P.astype(np.float32), T


def one_triangle():
    return np.array([[0.0, 0.0, 0.0], [0.05, 0.01, 0.0], [0.01, 0.04, 0.02]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def two_triangles():
    """two triangles sharing the edge 1-2, folded"""
    V = np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, 0.04, 0.0], [0.05, 0.04, 0.03]], dtype=np.float32)
    return V, np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)


def degenerate_list():
    """live triangles between degenerate ones: collinear vertices, a repeated index, a repeated vertex, NaN and infinite
    vertices; triangle 7 is live but far too small for a row (from float vertices no cross product underflows in fp64)"""
    V = np.array([[0.0, 0.0, 0.0], [0.03, 0.0, 0.0], [0.0, 0.03, 0.0], [0.06, 0.0, 0.0], [np.nan, 0.0, 0.0], [np.inf, 0.01, 0.0],
                  [0.03, 0.03, 0.02], [0.0, 0.0, 0.0], [1e-30, 0.0, 0.0], [0.0, 1e-30, 0.0], [0.0, -np.inf, 0.0]], dtype=np.float32)
    T = np.array([[0, 1, 3], [0, 1, 2], [1, 1, 2], [0, 7, 2], [0, 4, 2], [1, 6, 2], [0, 5, 1], [0, 8, 9], [2, 10, 6], [1, 3, 6]],
                 dtype=np.int32)
    return V, T


def all_degenerate():
    V, T = degenerate_list()
    return V, T[[0, 2, 3, 4, 6, 8]]


def boundary_triangle(extent_px, R=64):
    """a sliver along y whose box in the view along +z is ceil-to-floor `extent_px` pixels wide, between two small corner
    triangles that fix the mesh's box to +-0.1 (so one pixel is 0.2 sqrt(3) / (R - 2)); the sliver is triangle 2"""
    px = 0.2 * np.sqrt(3.0) / (R - 2)
    y0, y1 = (10.25 - R / 2) * px, (10.5 + extent_px - R / 2) * px  # X = y / px + R / 2: from 10.25 to 10.5 + extent_px
    e = 0.002
    V = np.array([[-0.1, -0.1, -0.1], [-0.1 + e, -0.1, -0.1], [-0.1, -0.1 + e, -0.1],
                  [0.1, 0.1, 0.1], [0.1 - e, 0.1, 0.1], [0.1, 0.1 - e, 0.1],
                  [0.0, y0, 0.0], [0.3 * px, y1, 0.0], [0.6 * px, y0, 0.0]], dtype=np.float32)
    return V, np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], dtype=np.int32)


def lone_triangle():
    """the largest box a triangle can have in a view: alone, its own box is the mesh's"""
    return np.array([[0.0, 0.0, 0.0], [0.2, 0.0, 0.0], [0.0, 0.2, 0.0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)
