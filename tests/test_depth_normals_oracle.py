"""The numpy oracle of ppf_cloud_from_depth_normals (tests/depth_normals_oracle.py) on the CPU: against a scalar restatement
one pixel at a time, the C1 frame's figures, an analytic plane and the threshold rule."""
import math

import numpy as np
import pytest

import depth_normals_oracle as O
import plane_oracle as P
import prep_data as D


@pytest.fixture(scope="module")
def c1():
    return D.c1_frame()


def scalar_xyz(z, u, v, intr, fp64):
    """one pixel's float32 x y z: depth_back_project in plain Python"""
    fx, fy, ppx, ppy = intr
    zf = np.float32(z)
    if fp64:
        return np.float32((u - ppx) * float(zf) / fx), np.float32((v - ppy) * float(zf) / fy), zf
    return np.float32(float(np.float32(u - ppx) * zf) / fx), np.float32(float(np.float32(v - ppy) * zf) / fy), zf


def scalar_pixel(z, keep, intr, fp64, v, u, radius, max_depth_change, min_neighbours):
    """(nx, ny, nz, curvature, k) of the kept pixel (u, v): plain loops in visiting order, plane_oracle's Jacobi"""
    H, W = z.shape
    zp = float(z[v, u])
    lim = float(np.float32(max_depth_change)) * zp
    nb = []
    for dv in range(-radius, radius + 1):
        for du in range(-radius, radius + 1):
            qv, qu = v + dv, u + du
            if 0 <= qv < H and 0 <= qu < W and keep[qv, qu] and math.fabs(float(z[qv, qu]) - zp) <= lim:
                nb.append(tuple(float(t) for t in scalar_xyz(z[qv, qu], qu, qv, intr, fp64)))
    k = len(nb)
    nan = np.float32(np.nan)
    if k < min_neighbours:
        return nan, nan, nan, nan, k
    c = [0.0, 0.0, 0.0]
    for q in nb:
        for a in range(3):
            c[a] += q[a]
    c = [t / float(k) for t in c]
    cov = [0.0] * 6
    for q in nb:
        d = [q[a] - c[a] for a in range(3)]
        for a, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            cov[a] += d[i] * d[j]
    cov = [t / float(k) for t in cov]
    trace = (cov[0] + cov[3]) + cov[5]
    n = P.jacobi_normal(cov)
    A = [[cov[0], cov[1], cov[2]], [cov[1], cov[3], cov[4]], [cov[2], cov[4], cov[5]]]   # the same sweeps again, for the eigenvalue
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(12):
        P._rotate(A, V, 0, 1)
        P._rotate(A, V, 0, 2)
        P._rotate(A, V, 1, 2)
    lam = A[0][0]
    if A[1][1] < lam:
        lam = A[1][1]
    if A[2][2] < lam:
        lam = A[2][2]
    p = [float(t) for t in scalar_xyz(z[v, u], u, v, intr, fp64)]
    if -((p[0] * n[0] + p[1] * n[1]) + p[2] * n[2]) < 0:
        n = -n
    curv = np.float32(math.fabs(lam) / math.fabs(trace)) if trace != 0.0 else np.float32(0)
    return np.float32(n[0]), np.float32(n[1]), np.float32(n[2]), curv, k


def test_oracle_equals_the_scalar_restatement_on_200_pixels(c1):
    _, depth, box, intr = c1
    z = O.metric_depth(depth)
    keep = O.keep_mask(z)
    vv, uu = np.nonzero(keep)
    rng = np.random.default_rng(2024)
    for fp64, radius, mdc, mn in ((True, 3, 0.02, 3), (False, 2, 0.01, 9)):
        rows, curv, k = O.depth_normals(depth, intr, fp64=fp64, radius=radius, max_depth_change=mdc, min_neighbours=mn, return_k=True)
        assert rows.shape == (vv.size, 6)
        pick = rng.choice(vv.size, size=100, replace=False)
        pick[:8] = np.argsort(k, kind="stable")[:8]     # the sparsest neighbourhoods are in, the ones without a normal too
        for i in pick:
            nx, ny, nz, cv, kk = scalar_pixel(z, keep, intr, fp64, int(vv[i]), int(uu[i]), radius, mdc, mn)
            want = np.array([*scalar_xyz(z[vv[i], uu[i]], int(uu[i]), int(vv[i]), intr, fp64), nx, ny, nz, cv], np.float32)
            got = np.concatenate([rows[i], curv[i:i + 1]])
            assert got.tobytes() == want.tobytes() and kk == k[i], (i, got, want, kk, k[i])


C1_TABLE = [  # radius, max_depth_change -> rows kept, rows without a normal, curvature > 0.03
    (3, 0.02, 166718, 12, 5000),
    (2, 0.02, 166718, 21, 4672),
    (5, 0.02, 166718, 5, 8674),
    (3, 0.01, 166718, 66, 5081),
]


@pytest.mark.parametrize("radius,mdc,n_rows,n_none,n_edge", C1_TABLE)
def test_c1_frame_figures(c1, radius, mdc, n_rows, n_none, n_edge):
    xyz, depth, box, intr = c1
    rows, curv = O.depth_normals(depth, intr, fp64=True, radius=radius, max_depth_change=mdc, min_neighbours=3)
    assert rows[:, :3].tobytes() == xyz.tobytes()
    none = np.isnan(curv)
    assert np.array_equal(none, np.isnan(rows[:, 3:]).all(axis=1)) and np.array_equal(none, np.isnan(rows[:, 3:]).any(axis=1))
    with np.errstate(invalid="ignore"):
        print(f"radius {radius} mdc {mdc}: rows {rows.shape[0]} none {int(none.sum())} edge {int((curv > 0.03).sum())}")
        assert (rows.shape[0], int(none.sum()), int((curv > 0.03).sum())) == (n_rows, n_none, n_edge)
    nrm = rows[~none, 3:].astype(np.float64)
    assert np.isfinite(nrm).all() and np.isfinite(curv[~none]).all()
    dev = np.abs(np.sqrt((nrm * nrm).sum(axis=1)) - 1.0).max()
    print(f"max | |n| - 1 | = {dev:.3g}")
    assert dev <= 1e-7
    dropped, dcurv = O.depth_normals(depth, intr, fp64=True, radius=radius, max_depth_change=mdc, min_neighbours=3, drop=True)
    assert dropped.tobytes() == rows[~none].tobytes() and dcurv.tobytes() == curv[~none].tobytes()


def plane_image(rows=48, cols=64, intr=(600.0, 610.0, 31.5, 23.25), normal=(0.2, -0.3, 0.93), offset=0.7):
    n = np.asarray(normal, np.float64)
    n /= np.linalg.norm(n)
    fx, fy, ppx, ppy = intr
    u, v = np.arange(cols)[None, :], np.arange(rows)[:, None]
    z = offset / (n[0] * (u - ppx) / fx + n[1] * (v - ppy) / fy + n[2])
    return z.astype(np.float32), intr, n


@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("radius", [1, 3, 8])
def test_analytic_plane(radius, fp64):
    img, intr, n = plane_image()
    rows, curv = O.depth_normals(img, intr, fp64=fp64, radius=radius, max_depth_change=0.5, min_neighbours=3)
    assert rows.shape[0] == img.size and not np.isnan(rows).any() and not np.isnan(curv).any()
    err = (1.0 - rows[:, 3:].astype(np.float64) @ (-n)).max()
    print(f"radius {radius} fp64 {fp64}: 1 - n.(-plane) <= {err:.3g}, curvature <= {curv.max():.3g}")
    assert err <= 1e-6 and curv.max() <= 1e-9


def threshold_image():
    return np.array([[1.0, 1.0, 1.0, 1.25, np.nextafter(np.float32(1.25), np.float32(2))]], np.float32)


def test_threshold_equality_is_a_neighbour_one_ulp_more_is_not():
    img = threshold_image()
    assert img[0, 4] > img[0, 3]
    _, _, k = O.depth_normals(img, (500.0, 500.0, 2.0, 0.0), radius=8, max_depth_change=0.25, min_neighbours=3, return_k=True)
    assert k.tolist() == [4, 4, 4, 5, 5]
