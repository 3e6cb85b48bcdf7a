"""tests/mesh_oracle.py, the numpy restatement of ppf_cloud_from_mesh's specification (include/ppf_hip.h):
against plain Python loops on the smallest meshes, then known answers that follow from the specification, then the
properties the stage exists for -- inner faces gone, outer faces whole, normals outward -- as conditions on the result."""
import functools
import math

import numpy as np
import pytest

import mesh_cases as MC
import mesh_oracle as MO


def f32(x):
    return float(np.float32(x))


def _mix(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _h(seed, k, c):
    return _mix(_mix(_mix((seed + 0x9E3779B9) & 0xFFFFFFFF) ^ k) ^ (c & 0xFFFFFFFF))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def loops(V, T, spacing, seed, R, min_views=0, depth_tol=0.0, orient=1, visibility=1):
    """the specification in scalar Python floats, one triangle, row, view and pixel at a time"""
    V = [[float(x) for x in v] for v in V]
    s = f32(spacing)
    tris, sampled = [], []
    for k, (i0, i1, i2) in enumerate(T):
        v0, e1, e2 = V[i0], [V[i1][a] - V[i0][a] for a in range(3)], [V[i2][a] - V[i0][a] for a in range(3)]
        c = _cross(e1, e2)
        L = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        assert L > 0 and math.isfinite(L)
        q = (0.5 * L) / (s * s)
        n = int(math.floor(q)) + ((_h(seed, k, 0) >> 8) < int(math.floor((q - math.floor(q)) * 16777216.0)))
        tris.append((i0, i1, i2))
        for j in range(n):
            u = ((_h(seed, k, 2 * j + 1) >> 8) + 0.5) / 16777216.0
            w = ((_h(seed, k, 2 * j + 2) >> 8) + 0.5) / 16777216.0
            if u + w > 1.0:
                u, w = 1.0 - u, 1.0 - w
            sampled.append([f32((v0[a] + u * e1[a]) + w * e2[a]) for a in range(3)] + [f32(c[a] / L) for a in range(3)])
    if not visibility:
        return np.array(sampled, dtype=np.float32).reshape(-1, 6), 0
    dirs = [[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
    pts = [V[i] for t in tris for i in t]
    lo, hi = [min(p[a] for p in pts) for a in range(3)], [max(p[a] for p in pts) for a in range(3)]
    ctr = [0.5 * (lo[a] + hi[a]) for a in range(3)]
    g = [hi[a] - lo[a] for a in range(3)]
    r = 0.5 * math.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    px = 2.0 * r / float(R - 2)
    tol = f32(depth_tol) if depth_tol > 0 else 2.0 * px
    seen, front, back = [0] * len(sampled), [0] * len(sampled), [0] * len(sampled)
    for dv in dirs:
        sc = 1.0 / math.sqrt(float(sum(1 for x in dv if x)))
        d = [float(x) * sc for x in dv]
        ax = min(range(3), key=lambda a: (abs(d[a]), a))
        t = _cross(d, [1.0 if a == ax else 0.0 for a in range(3)])
        tl = math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        av = [x / tl for x in t]
        bv = _cross(d, av)

        def proj(p):
            sft = [p[a] - ctr[a] for a in range(3)]
            return _dot(sft, av) / px + 0.5 * R, _dot(sft, bv) / px + 0.5 * R, _dot(sft, d) + r

        zmap = {}
        for tri in tris:
            (ax_, ay, az), (bx, by, bz), (cx, cy, cz) = [(X, Y, f32(D)) for X, Y, D in (proj(V[i]) for i in tri)]
            x0, x1 = max(math.ceil(min(ax_, bx, cx)), 0), min(math.floor(max(ax_, bx, cx)), R - 1)
            y0, y1 = max(math.ceil(min(ay, by, cy)), 0), min(math.floor(max(ay, by, cy)), R - 1)
            area = (bx - ax_) * (cy - ay) - (by - ay) * (cx - ax_)
            if area == 0.0:
                continue
            for j in range(y0, y1 + 1):
                for i in range(x0, x1 + 1):
                    w0 = (cx - bx) * (j - by) - (cy - by) * (i - bx)
                    w1 = (ax_ - cx) * (j - cy) - (ay - cy) * (i - cx)
                    w2 = (bx - ax_) * (j - ay) - (by - ay) * (i - ax_)
                    if (w0 >= 0 and w1 >= 0 and w2 >= 0) or (w0 <= 0 and w1 <= 0 and w2 <= 0):
                        z = f32(((w0 * az + w1 * bz) + w2 * cz) / area)
                        z = z if z > 0 else 0.0
                        zmap[(i, j)] = min(zmap.get((i, j), math.inf), z)  # floats >= 0 order as their bit patterns do
        for n, row in enumerate(sampled):
            X, Y, D = proj(row[:3])
            i, j = math.floor(X + 0.5), math.floor(Y + 0.5)
            vis = not (0 <= i < R and 0 <= j < R) or (i, j) not in zmap or f32(D) <= zmap[(i, j)] + tol
            if vis:
                sd = _dot(row[3:], d)
                seen[n] += 1
                front[n] += sd < 0
                back[n] += sd > 0
    out, flipped = [], 0
    for n, row in enumerate(sampled):
        if seen[n] >= max(1, min_views):
            if orient and back[n] > front[n]:
                row = row[:3] + [-x for x in row[3:]]
                flipped += 1
            out.append(row)
    return np.array(out, dtype=np.float32).reshape(-1, 6), flipped


@pytest.mark.parametrize("mesh,kw", [
    (MC.one_triangle, dict(spacing=0.004, seed=0, R=16)),
    (MC.one_triangle, dict(spacing=0.003, seed=5, R=24, min_views=3, depth_tol=0.001)),
    (MC.two_triangles, dict(spacing=0.004, seed=1, R=16)),
    (MC.two_triangles, dict(spacing=0.005, seed=2, R=32, orient=0)),
    (MC.two_triangles, dict(spacing=0.004, seed=3, R=16, visibility=0, orient=0)),
])
def test_the_oracle_equals_plain_loops(mesh, kw):
    V, T = mesh()
    want, flipped = loops(V, T, **kw)
    kw = dict(kw)
    got = MO.mesh_sample(V, T, kw.pop("spacing"), map_size=kw.pop("R"), **kw)
    assert len(want) > 20
    assert got["rows"].tobytes() == want.tobytes()
    assert got["stats"]["n_flipped"] == flipped


def test_the_hash_has_its_known_values():
    """h(seed, k, c) = mix(mix(mix(seed + 0x9e3779b9) ^ k) ^ c), the murmur3 finaliser: values computed by hand-run integer code"""
    assert int(MO.mix(1)) == _mix(1) == 0x514E28B7  # murmur3's fmix32(1)
    for s, k, c in [(0, 0, 0), (1, 2, 3), (0xFFFFFFFF, 7, 0xFFFFFFFF), (42, 1 << 31, 99)]:
        assert int(MO.mesh_hash(s, k, c)) == _h(s, k, c)
    assert _h(0, 0, 0) != 0
    got = MO.mesh_hash(3, np.arange(1000), 0)
    assert len(set(int(x) for x in got)) == 1000


def test_view_frames_are_orthonormal_and_ordered():
    d, a, b = MO.view_frames()
    assert d.shape == (26, 3)
    assert np.allclose(d[0], -np.ones(3) / np.sqrt(3)) and np.allclose(d[-1], np.ones(3) / np.sqrt(3))
    assert np.array_equal(d[12], [0.0, 0.0, -1.0]) and np.array_equal(d[13], [0.0, 0.0, 1.0])
    assert np.array_equal(a[13], [0.0, 1.0, 0.0]) and np.array_equal(b[13], [-1.0, 0.0, 0.0])
    for M in (d, a, b):
        assert np.allclose(np.linalg.norm(M, axis=1), 1.0, atol=1e-15)
    assert np.allclose(np.einsum("ij,ij->i", d, a), 0, atol=1e-15) and np.allclose(np.cross(d, a), b, atol=1e-15)


@functools.lru_cache(maxsize=None)
def _box(R, rot, inner):
    mesh = MC.box_in_box() if inner else MC.box()
    V, T = MC.rotated(mesh) if rot else mesh
    return V, T, MO.mesh_sample(V, T, 0.004, map_size=R)


def test_row_counts_are_floor_or_floor_plus_one():
    for V, T in (MC.box(), MC.torus(), MC.rotated(MC.box_in_box())):
        o = MO.mesh_sample(V, T, 0.004, visibility=0, orient=0)
        f = np.floor(o["q"]).astype(np.int64)
        assert ((o["n_k"] == f) | (o["n_k"] == f + 1)).all()
        assert o["stats"]["n_sampled"] == o["n_k"].sum() == len(o["rows"])
    V, T, o = _box(64, False, False)
    assert np.allclose(o["q"], [875] * 4 + [625] * 4 + [437.5] * 4, rtol=1e-6)  # 0.5 * 0.14 * 0.20 / 0.004^2 = 875, ...
    assert abs(o["stats"]["area"] - 2 * (0.10 * 0.14 + 0.14 * 0.20 + 0.10 * 0.20)) < 1e-8
    # the dither is fair: over many seeds a q of 437.5 rounds up about half the time
    ups = sum(int(MO.row_counts(np.array([2 * 437.5 * 0.004 ** 2]), np.array([True]), 0.004, s)[0][0] == 438) for s in range(400))
    assert 150 < ups < 250


def test_rows_lie_in_their_triangles():
    for V, T in (MC.rotated(MC.box()), MC.torus(nu=12, nv=8)):
        o = MO.mesh_sample(V, T, 0.003, visibility=0, orient=0, seed=4)
        v0, e1, e2, c, L, live = MO.triangles_geom(V, T)
        k = o["tri"]
        p = o["rows"][:, :3].astype(np.float64) - v0[k]
        n = c[k] / L[k][:, None]
        scale = np.abs(V[:, :3]).max()
        assert np.abs(np.einsum("ij,ij->i", p, n)).max() <= 4 * scale * 2.0 ** -24  # float rounding of three components
        # barycentric coordinates from the plane's own basis
        u = np.einsum("ij,ij->i", np.cross(p, e2[k]), c[k]) / (L[k] ** 2)
        w = np.einsum("ij,ij->i", np.cross(e1[k], p), c[k]) / (L[k] ** 2)
        eps = 1e-5
        assert (u >= -eps).all() and (w >= -eps).all() and (u + w <= 1 + eps).all()
        assert np.abs(np.linalg.norm(o["rows"][:, 3:].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_appending_triangles_leaves_earlier_rows_alone():
    V, T = MC.torus(nu=10, nv=6)
    a = MO.mesh_sample(V, T[:50], 0.003, visibility=0, orient=0, seed=9)
    b = MO.mesh_sample(V, T, 0.003, visibility=0, orient=0, seed=9)
    assert len(b["rows"]) > len(a["rows"]) > 50
    assert b["rows"][:len(a["rows"])].tobytes() == a["rows"].tobytes()


def test_each_seed_gives_another_cloud():
    V, T = MC.box()
    clouds = [MO.mesh_sample(V, T, 0.006, visibility=0, orient=0, seed=s)["rows"] for s in range(4)]
    for i in range(4):
        for j in range(i):
            assert clouds[i].shape[0] != clouds[j].shape[0] or not np.array_equal(clouds[i], clouds[j])
    again = MO.mesh_sample(V, T, 0.006, visibility=0, orient=0, seed=2)["rows"]
    assert again.tobytes() == clouds[2].tobytes()


def test_visibility_off_returns_every_sampled_row():
    V, T = MC.box_in_box()
    o = MO.mesh_sample(V, T, 0.004, visibility=0, orient=0)
    assert o["stats"]["n_rows"] == o["stats"]["n_sampled"] == len(o["sampled"]) and o["stats"]["n_hidden"] == 0
    assert o["rows"].tobytes() == o["sampled"].tobytes()
    assert set(o["tri"]) == set(range(24))


def test_degenerate_triangles_give_no_rows():
    V, T = MC.degenerate_list()
    o = MO.mesh_sample(V, T, 0.002, map_size=64)
    assert o["stats"]["n_degenerate"] == 6 and o["n_k"][7] == 0 and o["stats"]["n_triangles"] == 10
    assert set(o["sampled_tri"]) == {1, 5, 9}
    assert np.isfinite(o["rows"]).all() and len(o["rows"]) > 100
    V, T = MC.all_degenerate()
    o = MO.mesh_sample(V, T, 0.002, map_size=64)
    assert o["stats"]["n_degenerate"] == len(T) and o["stats"]["n_sampled"] == 0 and o["rows"].shape == (0, 6)
    assert o["stats"]["area"] == 0.0


def test_capacity():
    V, T = MC.box()
    with pytest.raises(MO.MeshCapacity):
        MO.mesh_sample(V, T, 0.004, max_rows=7000)
    with pytest.raises(MO.MeshCapacity):
        MO.mesh_sample(V, T, 0.004, max_rows=500)  # one triangle's q alone
    assert MO.mesh_sample(V, T, 0.004, max_rows=8000, visibility=0, orient=0)["stats"]["n_sampled"] <= 8000


def test_the_boundary_cases_have_the_boxes_they_are_named_for():
    for extent in (16, 17):
        V, T = MC.boundary_triangle(extent)
        o = MO.mesh_sample(V, T, 0.002, map_size=64)
        assert o["sides"][13, 2, 0] == extent  # the view along +z maps y to X
        assert o["sides"][:, 2, :].max() == extent
        assert (o["stats"]["n_large"] > 0) == (extent > MO.SMALL_PX)


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("R", [64, 128, 256])
def test_box_in_box_loses_its_inside_and_turns_outward(R, rot):
    """spacing 4 mm, the default depth_tol: no row of an inner triangle survives, every row of an outer triangle does, and
    every surviving normal points away from the centre although half the outer windings were reversed"""
    V, T, o = _box(R, rot, True)
    inner = o["sampled_tri"] >= 12
    assert inner.sum() > 2000 and (~inner).sum() > 7000
    assert not o["keep"][inner].any(), f"{o['keep'][inner].sum()} inner rows survive"
    assert o["keep"][~inner].all(), f"{(~o['keep'][~inner]).sum()} outer rows are lost"
    ctr = 0.5 * (V[:, :3].astype(np.float64).min(axis=0) + V[:, :3].astype(np.float64).max(axis=0))
    out = np.einsum("ij,ij->i", o["rows"][:, 3:].astype(np.float64), o["rows"][:, :3].astype(np.float64) - ctr)
    assert (out > 0).all()
    assert o["stats"]["n_flipped"] == (o["sampled_tri"][o["keep"]] % 2 == 1).sum()  # exactly the rows of the reversed triangles


@pytest.mark.parametrize("R", [128, 256])
def test_the_torus_keeps_every_row_and_flips_none(R):
    V, T = MC.torus(nu=48, nv=24)
    o = MO.mesh_sample(V, T, 0.003, map_size=R)
    assert o["stats"]["n_sampled"] > 5000
    assert o["stats"]["n_hidden"] == 0 and o["stats"]["n_flipped"] == 0
