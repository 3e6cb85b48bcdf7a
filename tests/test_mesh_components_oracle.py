"""tests/mesh_components_oracle.py against itself, against meshes whose answers are known and on the project's scenes, on the
CPU: the vectorised oracle equals plain loops; the hand-made meshes; the fused sphere, render_scan's two objects and the
analytic sphere; and the condition the device test's loop relies on: min_triangles = 100 keeps exactly the scan's two objects."""
import numpy as np

import mesh_components_oracle as MC

F32, F64 = np.float32, np.float64
HAND = MC.hand_made()
PARAMS = [dict(), dict(min_triangles=2), dict(min_area=0.5), dict(rank_lo=1, rank_hi=2), dict(rank_lo=1, rank_hi=1),
          dict(min_triangles=3, rank_hi=2)]


def one(name, **kw):
    return MC.components(*HAND[name], **kw)


def test_vectorised_oracle_equals_plain_loops():
    meshes = [MC.random_mesh(40, 12, 0), MC.random_mesh(40, 30, 1), MC.random_mesh(40, 200, 2), MC.random_mesh(7, 3, 3, normals=False),
              MC.strip(50, 4), MC.fan(9), MC.isolated(11), MC.sized(65)] + list(HAND.values())
    seen = set()
    for n, (v, t) in enumerate(meshes):
        for kw in PARAMS:
            a, b = MC.components(v, t, **kw), MC.components_loops(v, t, **kw)
            assert MC.same(a, b) == [], (n, kw, MC.same(a, b))
        seen.add(a["n_components"])
    assert {0, 1} < seen and max(seen) > 5


def test_one_triangle():
    r = one("one triangle")
    i = r["info"][0]
    assert r["n_components"] == 1 and (i["n_vertices"], i["n_triangles"], i["n_edges"], i["n_boundary_edges"]) == (3, 1, 3, 3)
    assert i["area"] == 0.5 and i["kept"] == 1 and i["first_vertex"] == 0 and MC.euler(i) == 1
    assert i["lo"].tolist() == [0, 0, 0] and i["hi"].tolist() == [1, 1, 0] and r["labels"].tolist() == [0, 0, 0]


def test_two_triangles_sharing_an_edge_or_a_vertex():
    i = one("shared edge")["info"]
    assert len(i) == 1 and (i[0]["n_edges"], i[0]["n_boundary_edges"], i[0]["n_nonmanifold_edges"]) == (5, 4, 0) and i[0]["area"] == 1.0
    i = one("shared vertex")["info"]
    assert len(i) == 1 and (i[0]["n_edges"], i[0]["n_boundary_edges"], i[0]["n_vertices"]) == (6, 6, 5)


def test_a_closed_tetrahedron():
    i = one("tetrahedron")["info"]
    assert len(i) == 1 and (i[0]["n_edges"], i[0]["n_boundary_edges"], i[0]["n_nonmanifold_edges"]) == (6, 0, 0) and MC.euler(i[0]) == 2


def test_three_triangles_on_one_edge():
    i = one("three on an edge")["info"]
    assert len(i) == 1 and (i[0]["n_edges"], i[0]["n_nonmanifold_edges"], i[0]["n_boundary_edges"]) == (7, 1, 6)


def test_a_degenerate_triangle_bridges_two_pieces():
    v, t = HAND["degenerate bridge"]
    assert MC.components(v, t[:2])["n_components"] == 2
    r = MC.components(v, t)
    i = r["info"][0]
    assert r["n_components"] == 1 and (i["n_triangles"], i["n_degenerate"], i["n_edges"], i["n_vertices"]) == (3, 1, 6, 6)
    assert i["area"] == 1.0 and r["n_bad_area"] == 0


def test_an_unreferenced_vertex():
    r = one("unreferenced vertex")
    assert r["n_unreferenced"] == 2 and r["labels"].tolist() == [-1, 0, 0, 0, -1] and r["info"][0]["first_vertex"] == 1
    assert r["out_vertices"].tobytes() == MC.as_mesh(*HAND["unreferenced vertex"])[0][1:4].tobytes()
    assert r["out_triangles"].tolist() == [[0, 1, 2]] and r["info"][0]["hi"].tolist() == [1, 1, 0]
    r = one("vertices only")
    assert (r["n_components"], r["n_unreferenced"], r["n_vertices_out"]) == (0, 3, 0) and r["labels"].tolist() == [-1, -1, -1]
    r = one("empty")
    assert all(r[k] == 0 for k in MC.COUNTS) and r["out_vertices"].shape == (0, 6) and r["out_triangles"].shape == (0, 3)


def test_a_huge_coordinate_has_no_integer_area():
    r = one("huge coordinate")
    assert r["n_bad_area"] == 1 and r["n_components"] == 2
    # the triangle of area 0.5 ranks before the one whose area could not be counted
    assert r["info"]["area"].tolist() == [0.5, 0.0] and r["info"]["first_vertex"].tolist() == [3, 0]


def test_congruent_pieces_rank_by_first_vertex():
    r = one("congruent pieces")
    i = r["info"]
    assert i["area"].tolist() == [0.5, 0.125, 0.125] and i["first_vertex"].tolist() == [12, 0, 6]
    assert i["n_triangles"].tolist() == [1, 4, 4]
    r = one("congruent pieces", rank_lo=1, rank_hi=2)
    assert r["info"]["kept"].tolist() == [0, 1, 0] and r["n_vertices_out"] == 6 and r["out_triangles"].max() == 5
    # min_area at exactly the area keeps, one ulp above does not
    assert one("congruent pieces", min_area=0.125)["n_kept"] == 3
    assert one("congruent pieces", min_area=np.nextafter(F32(0.125), F32(1)))["n_kept"] == 1


def test_signed_zeros_order():
    i = one("signed zeros")["info"][0]
    assert np.signbit(i["lo"]).tolist() == [True, True, False] and np.signbit(i["hi"]).tolist() == [False, False, False]


def test_everything_kept_is_the_input():
    for name in ("tetrahedron", "congruent pieces", "degenerate bridge"):
        v, t = MC.as_mesh(*HAND[name])
        r = MC.components(v, t)
        assert r["out_vertices"].tobytes() == v.tobytes() and r["out_triangles"].tobytes() == t.tobytes(), name


def test_the_fused_sphere():
    r = MC.scene_components("sphere")
    v, t = MC.scene_mesh("sphere")
    i = r["info"]
    print(f"fused sphere: {len(v)} vertices, {len(t)} triangles, {r['n_components']} components; largest {i[0]}; "
          f"scraps of {i['n_triangles'][1:].min()} .. {i['n_triangles'][1:].max()} triangles")
    assert (len(v), len(t)) == (11284, 21228) and r["n_components"] == 26 and r["n_unreferenced"] == 0 and r["n_bad_area"] == 0
    assert i[0]["n_triangles"] == 20746 and i[0]["n_boundary_edges"] == 1024 and MC.euler(i[0]) == -37
    # the issue's prototype gave scraps of 8 .. 62 triangles; this oracle finds two of 2 triangles as well
    assert i["n_triangles"][1:].min() == 2 and i["n_triangles"][1:].max() == 62 and i["n_triangles"][1:].sum() == 21228 - 20746
    assert i["n_nonmanifold_edges"].sum() == 0 and i["n_degenerate"].sum() == 0


def test_the_scan_of_two_objects():
    r = MC.scene_components("scan")
    v, t = MC.scene_mesh("scan")
    i = r["info"]
    print(f"scan: {len(v)} vertices, {len(t)} triangles, {r['n_components']} components; {i[0]}; {i[1]}; the rest: "
          f"{int(i['n_triangles'][2:].sum())} triangles, the largest of {i['n_triangles'][2:].max()} and {i['area'][2:].max():.3g} m^2")
    assert (len(v), len(t)) == (7280, 13530) and r["n_components"] == 29
    assert i["n_triangles"][:2].tolist() == [7244, 6008] and i["n_triangles"][2:].max() <= 24 and i["n_triangles"][2:].sum() == 278
    assert abs(i[0]["area"] - 0.02084) < 5e-6 and abs(i[1]["area"] - 0.01710) < 5e-6 and i["area"][2:].max() < 6.1e-5
    # the sphere lies at x < 0, the ellipsoid at x > 0
    assert i[0]["hi"][0] < 0.01 and i[1]["lo"][0] > 0.01
    # what the device test's loop relies on
    k = MC.components(v, t, min_triangles=100)
    assert k["info"]["kept"].tolist() == [1, 1] + [0] * 27 and k["n_triangles_out"] == 7244 + 6008


def test_the_analytic_sphere_is_one_closed_component():
    import depth_volume_oracle as O
    import volume_mesh_oracle as M
    voxel, rad, trunc = 0.010, 0.035, 0.040
    vol = O.Volume((12, 13, 14), voxel, (0.0, 0.0, 0.0), trunc)
    centre = np.array([0.0573, 0.0612, 0.0664])
    c = vol.centres()
    P = np.meshgrid(c[2], c[1], c[0], indexing="ij")[::-1]
    dist = np.sqrt((P[0] - centre[0]) ** 2 + (P[1] - centre[1]) ** 2 + (P[2] - centre[2]) ** 2)
    vol.d = np.clip((dist - rad) / float(F32(trunc)), -1.0, 1.0).astype(F32)
    vol.w = np.ones(vol.d.shape, np.int32)
    v, t, _ = M.mesh(vol, 1)
    r = MC.components(v, t)
    i = r["info"][0]
    assert r["n_components"] == 1 and i["n_boundary_edges"] == 0 and i["n_nonmanifold_edges"] == 0 and MC.euler(i) == 2
    assert abs(i["area"] / (4 * np.pi * rad * rad) - 1) < 0.05
    assert r["out_vertices"].tobytes() == v.tobytes() and r["out_triangles"].tobytes() == t.tobytes()


def test_the_random_volumes():
    for which, want in ((((33, 9, 6), 1), (2961, 3996, 39)), (((17, 16, 3), 0), (1056, 1324, 26))):
        v, t = MC.scene_mesh(which)
        assert (len(v), len(t), MC.scene_components(which)["n_components"]) == want
