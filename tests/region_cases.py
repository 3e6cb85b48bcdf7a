"""Hand-made clouds for ppf_prep_regions that the CPU tests of tests/region_oracle.py and the device tests share: (n, 6) float32
rows x y z nx ny nz, a float32 curvature per row and the parameters they are meant for."""
import numpy as np

Z, X = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
THR = np.float32(0.03)                                     # the default curvature threshold
ROUGH = np.float32(0.5)                                    # a curvature far above it: a border row


def rows6(xyz, normal=Z):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    r = np.zeros((xyz.shape[0], 6), np.float32)
    r[:, :3] = xyz
    r[:, 3:] = np.asarray(normal, np.float32)
    return r


def smooth(n):
    return np.zeros(n, np.float32)


def random_cloud(n, seed, side=1.0, border_share=0.3, nan_share=0.02):
    """uniform rows in a cube, unit normals in every direction, curvatures on both sides of 0.03, a few non-finite values"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    rows = np.concatenate([rng.uniform(0, side, (n, 3)), v / np.linalg.norm(v, axis=1, keepdims=True)], axis=1).astype(np.float32)
    curv = np.where(rng.uniform(size=n) < border_share, rng.uniform(0.031, 0.3, n), rng.uniform(0, 0.03, n)).astype(np.float32)
    k = int(n * nan_share)
    rows[rng.integers(0, max(n, 1), k), rng.integers(0, 6, k)] = np.nan
    curv[rng.integers(0, max(n, 1), k)] = np.nan
    return rows, curv


def patches(n, seed, tol=0.02, degree=6.0, border_share=0.2):
    """n uniform rows in a cube of a mean degree of `degree` at `tol`, each with one of three normals and a curvature below or
    above 0.03: regions and loose rows of every size"""
    rng = np.random.default_rng(seed)
    side = (n * 4.0 / 3.0 * np.pi * tol ** 3 / degree) ** (1.0 / 3.0) if n else 1.0
    rows = rows6(rng.uniform(0, side, (n, 3)))
    rows[:, 3:] = np.array([Z, X, (0.0, 0.6, 0.8)], np.float32)[rng.integers(0, 3, n)]
    curv = np.where(rng.uniform(size=n) < border_share, ROUGH, np.float32(0.01)).astype(np.float32)
    return rows, curv


def grid_patch(nu, nv, pitch, origin, u, v, normal):
    """nu x nv rows on the plane through origin spanned by the unit vectors u, v"""
    a, b = np.meshgrid(np.arange(nu) * pitch, np.arange(nv) * pitch, indexing="ij")
    return rows6(np.asarray(origin) + a.reshape(-1, 1) * np.asarray(u) + b.reshape(-1, 1) * np.asarray(v), normal)


def perpendicular_planes(pitch=0.004, side=25):
    """a floor (z = 0, normal +z) and a wall (x = 0, normal +x) that meet in the edge x = z = 0: one cluster at tolerance 0.01,
    two regions.  625 floor rows, then 600 wall rows (the wall starts one pitch above the floor)"""
    floor = grid_patch(side, side, pitch, (0, 0, 0), (1, 0, 0), (0, 1, 0), Z)
    wall = grid_patch(side, side - 1, pitch, (0, 0, pitch), (0, 1, 0), (0, 0, 1), X)
    rows = np.concatenate([floor, wall])
    return rows, smooth(rows.shape[0])


def cosine_threshold():
    """pairs 0.005 apart (tolerance 0.01), far from each other: one normal is an axis, (0, 0, 1) or (0, 0, -1), the other
    (0.6, 0, nz) with nz float32(0.8), its float32 neighbours and their negatives, so the fp64 dot product is nz or -nz
    exactly: equal to normal_cos = float32(0.8), one float32 step to either side of it, or negative.
    Returns (rows, curv, normal_cos, per pair whether it is linked)"""
    c = np.float32(0.8)
    below, above = np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(1))
    rows, linked = [], []
    for k, (nz, sign) in enumerate([(c, 1), (below, 1), (above, 1), (c, -1), (-c, -1), (-c, 1), (-below, -1)]):
        a = rows6([[0.1 * k, 0, 0]], (0, 0, sign))
        b = rows6([[0.1 * k + 0.005, 0, 0]], (0.6, 0, nz))
        rows += [a, b]
        linked.append(float(nz) * sign >= float(c))
    rows = np.concatenate(rows)
    return rows, smooth(rows.shape[0]), float(c), linked


def curvature_threshold():
    """three rows in a line 0.005 apart: curvature exactly the threshold (smooth), one ulp above (a border row, attached),
    NaN (a border row too).  Returns (rows, curv)"""
    rows = rows6([[0, 0, 0], [0.005, 0, 0], [0.010, 0, 0]])
    return rows, np.array([THR, np.nextafter(THR, np.float32(1)), np.nan], np.float32)


def border_cases():
    """the border rules, one group of rows per y.  Returns (rows, curv, the labels at tolerance 0.01, min_size 1)"""
    rows, curv, want = [], [], []
    # y = 0: smooth rows 0 and 1 at x = 0 and 0.012 (not near each other); border row 2 at x = 0.007: 0.007 from row 0, 0.005
    # from row 1: the nearest wins -> row 1's region
    rows += [[0, 0, 0], [0.012, 0, 0], [0.007, 0, 0]]
    curv += [0, 0, ROUGH]
    # y = 1: smooth rows 3 and 4 at x = -0.006 and 0.006, border row 5 at x = 0 exactly between: the smaller index wins -> row 3's
    rows += [[-0.006, 1, 0], [0.006, 1, 0], [0, 1, 0]]
    curv += [0, 0, ROUGH]
    # y = 2: border row 6 alone with a smooth row 7 that is 0.02 away: no attachment
    rows += [[0, 2, 0], [0.02, 2, 0]]
    curv += [ROUGH, 0]
    # y = 3: smooth rows 8 and 10 0.016 apart with border rows 9 and 11 between them (0.004 apart, near each other and near both):
    # border rows carry no link, so 8 and 10 stay two regions; 9 joins 8, 11 joins 10
    rows += [[0, 3, 0], [0.006, 3, 0], [0.016, 3, 0], [0.010, 3, 0]]
    curv += [0, ROUGH, 0, ROUGH]
    # y = 4: border row 12 whose only near smooth row (13) disagrees in normal: no attachment; set below
    rows += [[0, 4, 0], [0.004, 4, 0]]
    curv += [ROUGH, 0]
    r = rows6(rows)
    r[13, 3:] = X
    # regions (smooth + attached): {1, 2}, {3, 5}, {8, 9}, {10, 11} of two rows, ranked by first row; then {0}, {4}, {7}, {13}
    want = np.array([4, 0, 0, 1, 5, 1, -1, 6, 2, 2, 3, 3, -1, 7], np.int32)
    return r, np.array(curv, np.float32), want


def two_cells_apart(disagree=False):
    """two crowded cells two cells apart at tolerance 0.02 (700 and 900 rows: three and four LDS tiles) that one pair of rows,
    the last of each, links: 0.0197 apart, every other pair at least 0.028.  disagree: the second cell's normals are +x"""
    rng = np.random.default_rng(0)
    a = (rng.uniform(0, 0.001, (700, 3)) + [0.0, 0.0, 1.0]).astype(np.float32)
    b = (rng.uniform(0, 0.001, (900, 3)) + [0.03, 0.0, 1.0]).astype(np.float32)
    a[699], b[899] = [0.0055, 0.0, 1.0], [0.0252, 0.0, 1.0]
    rows = np.concatenate([rows6(a), rows6(b, X if disagree else Z)])
    return rows, smooth(1600)


def alternating_plane(side=30, pitch=0.004):
    """a plane whose normals alternate between +z and -z like a chessboard: neighbours 0.004 apart disagree, the diagonal
    neighbours (0.00566 apart) agree: two regions at tolerance 0.01, one with PPF_REGION_UNORIENTED"""
    rows = grid_patch(side, side, pitch, (0, 0, 1), (1, 0, 0), (0, 1, 0), Z)
    i, j = np.divmod(np.arange(side * side), side)
    rows[(i + j) % 2 == 1, 5] = -1.0
    return rows, smooth(side * side)
