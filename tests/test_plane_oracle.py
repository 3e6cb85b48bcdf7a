"""tests/plane_oracle.py, the numpy restatement of ppf_prep_planes that the device is held to byte for byte,
against things that do not depend on it: the tree sum against math.fsum, the Jacobi normal against numpy.linalg.eigh,
synthetic planes with a known normal and offset, the rendered two-bottle frame whose background is a known plane, and the
rules of the specification (the three statuses, invalid hypotheses, rows behind a plane, apply == remove)."""
import math

import numpy as np
import pytest

import plane_oracle as P
import prep_data as D


def test_tree_sum_against_fsum():
    rng = np.random.default_rng(0)
    assert P.tsum([]) == 0.0
    for n in (1, 2, 63, 64, 65, 4095, 4096, 4097, 10000, 262145):   # the tree's boundaries lie at 64, 4,096 and 262,144 values
        v = rng.uniform(0.1, 2.0, n) * 10.0 ** rng.integers(-3, 4, n)
        want = math.fsum(v)
        assert abs(P.tsum(v) - want) <= 1e-12 * want, n
    # the tree is what the specification says: 64 + 1 values are two groups of the first level, then one of the second
    v = rng.normal(size=65)
    first = v[:64].copy()
    for off in (32, 16, 8, 4, 2, 1):
        first[:off] = first[:off] + first[off:2 * off]
    assert P.tsum(v) == (first[0] + (v[64] + 0.0))


def test_jacobi_normal_against_eigh():
    rng = np.random.default_rng(1)
    for _ in range(50):
        pts = rng.normal(size=(200, 3)) * rng.uniform(0.001, 1.0, 3)
        pts = pts @ np.linalg.qr(rng.normal(size=(3, 3)))[0]
        C = np.cov(pts.T, bias=True)
        n = P.jacobi_normal([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])
        w, V = np.linalg.eigh(C)
        want = V[:, 0]
        assert abs(np.linalg.norm(n) - 1.0) < 1e-12
        assert min(np.abs(n - want).max(), np.abs(n + want).max()) < 1e-12


def test_an_exact_plane_is_recovered():
    for seed, normal, offset in ((0, (0.2, -0.3, 0.93), 0.7), (1, (0.0, 0.0, -1.0), 1.2), (2, (-0.6, 0.1, 0.3), 0.4)):
        cloud, nrm = D.plane_cloud(seed=seed, normal=normal, offset=offset, noise=0.0)
        out, _, info, labels = P.remove_planes(cloud)
        row = info[0]
        assert row["status"] == P.REMOVED and row["n_rows"] == 1500 and row["n_inliers"] == 1500 and out.shape[0] == 0
        assert (labels == 1).all()
        assert row["d"] >= 0 and abs(np.linalg.norm(row["n"]) - 1.0) < 1e-12
        # n.p + d = 0 with d >= 0: the generating plane is nrm.p = offset, so n = -nrm, d = offset
        assert np.abs(row["n"] + nrm).max() < 1e-6 and abs(row["d"] - offset) < 1e-6


def test_a_noisy_plane_among_outliers():
    """3,000 plane rows with 1 mm noise and 1,000 rows of a sphere, shuffled.  Measured with this oracle: the normal is off
    by 4.87e-4 rad and no plane row is kept (5 sigma is the threshold); the bounds are twice that."""
    plane, nrm = D.plane_cloud(n=3000, seed=0, noise=0.001)
    sphere, _ = D.sphere_cloud(n=1000, seed=10)
    perm = np.random.default_rng(0).permutation(4000)
    cloud, is_plane = np.concatenate([plane, sphere])[perm], perm < 3000
    out, _, info, labels = P.remove_planes(cloud)
    err = math.acos(min(1.0, abs(float(info[0]["n"] @ nrm))))
    kept = float((labels[is_plane] == 0).mean())
    print(f"normal error {err:.3e} rad, share of plane rows kept {kept:.4f}, sphere rows removed {(labels[~is_plane] != 0).sum()}")
    assert info[0]["status"] == P.REMOVED and info[0]["refit"] == 1
    assert err <= 2 * 4.87e-4 and kept <= 2 * 0.0
    assert (labels[~is_plane] == 0).all() and out.shape[0] == 1000 + int(kept * 3000)


@pytest.fixture(scope="module")
def rendered(bottle_rows):
    from test_gpu_frame import _render_frame
    scene, depth, boxes, K, objs, solid = _render_frame(bottle_rows)
    # the background is the plane nrm.p = off of _render_frame; a pixel an object was drawn over lies in front of it
    nrm, off = np.array([0.1, -0.15, -1.0]) / np.linalg.norm([0.1, -0.15, -1.0]), -0.95
    background = np.abs(scene.astype(np.float64) @ nrm - off) < 1e-5
    return scene, background


@pytest.fixture(scope="module")
def bottle_rows():
    import os
    return np.load(os.path.join(D.GOLDEN, "bottle_model_xyzn.npy"))


@pytest.mark.parametrize("flags", [0, P.NO_REFIT], ids=["refit", "hypothesis"])
def test_rendered_frame_loses_exactly_its_background(rendered, flags):
    scene, background = rendered
    assert int(background.sum()) == 212390 and scene.shape[0] == 230400
    out, _, info, labels = P.remove_planes(scene, dict(flags=flags))
    assert info[0]["status"] == P.REMOVED and info[0]["refit"] == (0 if flags else 1)
    assert info[0]["n_rows"] == 230400 and info[0]["n_inliers"] == 212390
    np.testing.assert_array_equal(labels != 0, background)
    assert out.shape[0] == 18010
    np.testing.assert_array_equal(out, scene[~background])


def test_every_status_occurs():
    plane, _ = D.plane_cloud(n=1500, seed=3, offset=0.9)   # clear of the sphere
    sphere, _ = D.sphere_cloud(n=2000, seed=4, radius=0.15)
    # REMOVED, then REJECTED (a 1 cm slab holds at most a thirtieth of a sphere of 15 cm radius), then NONE
    _, _, info, _ = P.remove_planes(np.concatenate([plane, sphere]), dict(max_planes=3))
    assert list(info["status"]) == [P.REMOVED, P.REJECTED, P.NONE]
    assert info[1]["n_rows"] == 2000 and info[1]["n_inliers"] == 0 and 0 < info[1]["n_hyp_inliers"] < 200
    assert info[2].tobytes() == bytes(P.INFO.itemsize)
    # REMOVED, then NONE because fewer than three rows are left
    _, _, info, labels = P.remove_planes(np.concatenate([plane, sphere[:2]]), dict(max_planes=2))
    assert list(info["status"]) == [P.REMOVED, P.NONE] and list(labels[-2:]) == [0, 0]
    for n in (0, 1, 2):
        out, _, info, _ = P.remove_planes(plane[:n])
        assert info[0].tobytes() == bytes(P.INFO.itemsize) and out.shape[0] == n


def test_identical_rows_make_every_hypothesis_invalid():
    cloud = np.tile(np.array([[0.1, 0.2, 0.9]], np.float32), (500, 1))
    assert np.isnan(P.hypotheses(cloud.astype(np.float64), 1, 0, 64)).all()
    out, _, info, labels = P.remove_planes(cloud, dict(n_hypotheses=64))
    row = info[0]
    assert row["status"] == P.REJECTED and row["hypothesis"] == 0 and row["n_hyp_inliers"] == 0 and row["n_rows"] == 500
    assert not row["n"].any() and row["d"] == 0.0 and out.shape[0] == 500 and not labels.any()


def test_rows_behind_a_plane():
    plane, nrm = D.plane_cloud(n=2000, seed=5)
    rng = np.random.default_rng(6)
    front = (plane[:300].astype(np.float64) - rng.uniform(0.02, 0.2, (300, 1)) * nrm).astype(np.float32)   # towards the origin
    back = (plane[300:500].astype(np.float64) + rng.uniform(0.02, 0.2, (200, 1)) * nrm).astype(np.float32)
    bad = np.array([[np.nan, 0, 1], [0, -np.inf, 1], [0, 0, np.inf]], np.float32)
    cloud = np.concatenate([plane, front, back, bad])
    p = dict(flags=P.REMOVE_BEHIND)
    out, _, info, labels = P.remove_planes(cloud, p)
    assert info[0]["n_inliers"] == 2000 and info[0]["n_behind"] == 200
    assert (labels[:2000] == 1).all() and (labels[2000:2300] == 0).all() and (labels[2300:2500] == 0x81).all() and (labels[2500:] == 0).all()
    s = P.signed(list(info[0]["n"]) + [info[0]["d"]], *cloud[labels == 0x81].astype(np.float64).T)
    thr = float(np.float32(0.005))
    assert (s < -thr).all() and not (np.abs(s) <= thr).any()
    np.testing.assert_array_equal(out.view(np.uint32), cloud[labels == 0].view(np.uint32))
    # without the flag the rows behind the plane stay
    _, _, info0, labels0 = P.remove_planes(cloud)
    assert info0[0]["n_behind"] == 0 and (labels0[2300:2500] == 0).all()


@pytest.mark.parametrize("flags", [0, P.REMOVE_BEHIND, P.NO_REFIT])
def test_apply_to_the_cloud_itself_is_the_removal(flags):
    rng = np.random.default_rng(7)
    planes = [D.plane_cloud(n=1200, seed=s, normal=nv, offset=o, noise=0.0005)[0]
              for s, nv, o in ((8, (0, 0, -1.0), 0.9), (9, (0, -1.0, -0.2), 0.5), (10, (1.0, 0.1, -0.3), 0.45))]
    cloud = np.concatenate(planes + [D.sphere_cloud(n=800, seed=11)[0]])[rng.permutation(4400)]
    p = dict(max_planes=4, flags=flags)
    out, _, info, labels = P.remove_planes(cloud, p)
    assert (info["status"] == P.REMOVED).sum() >= 2
    keep = P.apply_planes(cloud, info, p)
    np.testing.assert_array_equal(keep, labels == 0)
    np.testing.assert_array_equal(cloud[keep], out)
