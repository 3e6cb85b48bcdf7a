"""tests/depth_volume_oracle.py (the numpy restatement of ppf_depth_volume the device tests compare bytes with) held to plain
per-voxel and per-pixel loops on a 5 x 4 x 3 volume, to known answers, and to the accuracy DESIGN.md §30 states.  No GPU.

Measured with the oracle (the asserted bounds are twice these, as §28 set its bounds):
  one frame integrated at the identity and raycast from it, against the input (SCENE_VOLUME, 10 mm voxels):
      median 2.5 mm, rms 34.2 mm, worst 392 mm (the rms and the worst are the silhouettes, where the ray meets the wall behind),
      87.9 % of the input's pixels come back
  four frames of cases.stream(4, 3, 20, 2) fused at their true poses, raycast against the exact image:
      views seen: rms <= 30.6 mm, median <= 0.56 mm, >= 92.8 % of the truth's pixels hit; a view not seen: 25.8 mm, 92.8 %
  the sphere of 0.1 m at 0.7 m, four views, 64^3 voxels of 5 mm: raycast rms <= 3.5 mm with >= 99.1 % hit; the extracted rows
      lie 0.72 mm rms and 4.8 mm worst from the sphere, their normals within acos(0.81) of the radial direction
  cases.stream(4, 5, 20, 2): the fused chain ends 0.86 mm / 0.019 deg from the truth, the frame-to-frame chain 0.35 mm / 0.030
      deg: on four frames and 10 mm voxels the model is no better than the chain; the ratio is recorded, not fixed."""
import numpy as np
import pytest

import depth_motion_oracle as MO
import depth_volume_cases as VC
import depth_volume_oracle as O

cases = O.cases
F32, F64 = np.float32, np.float64
INTR = cases.intrinsics()


# ---- the same arithmetic by plain loops ---------------------------------------------------------------------------------
def tiny_volume(seed=0, observed=0.8):
    """a 5 x 4 x 3 volume with random records: d in (-1, 1), w in 0..3"""
    rng = np.random.default_rng(seed)
    vol = O.Volume((5, 4, 3), 0.02, (-0.04, -0.03, 0.60), trunc=0.05, max_weight=3)
    vol.d = rng.uniform(-1, 1, vol.d.shape).astype(F32)
    vol.w = np.where(rng.random(vol.d.shape) < observed, rng.integers(1, 4, vol.d.shape), 0).astype(np.int32)
    vol.d[vol.w == 0] = F32(1)
    return vol


def integrate_loops(vol, img, intr, pose, depth_scale=0.001, z_min=0.0, z_max=0.0):
    fx, fy, ppx, ppy = (float(v) for v in intr)
    T = np.asarray(pose, F64).reshape(4, 4).tolist()
    z = O.level0(img, depth_scale, z_min, z_max)
    rows, cols = z.shape
    nx, ny, nz = vol.dims
    v, tr = float(vol.voxel), float(vol.trunc)
    n = 0
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                P = [vol.origin[0] + float(i) * v, vol.origin[1] + float(j) * v, vol.origin[2] + float(k) * v]
                p = [((T[r][0] * P[0] + T[r][1] * P[1]) + T[r][2] * P[2]) + T[r][3] for r in range(3)]
                if not p[2] > 0:
                    continue
                uf = np.floor((p[0] * fx / p[2] + ppx) + 0.5)
                vf = np.floor((p[1] * fy / p[2] + ppy) + 0.5)
                if not (0 <= uf < cols and 0 <= vf < rows):
                    continue
                zp = z[int(vf), int(uf)]
                if not zp > 0:
                    continue
                sdf = float(zp) - p[2]
                if sdf < -tr:
                    continue
                dn = min(sdf / tr, 1.0)
                d, w = float(vol.d[k, j, i]), int(vol.w[k, j, i])
                vol.d[k, j, i] = F32((d * float(w) + dn) / float(w + 1))
                vol.w[k, j, i] = min(w + 1, vol.max_weight)
                n += 1
    return n


def near_scalar(vol, P, min_weight):
    nx, ny, nz = vol.dims
    idx = [np.floor((P[a] - vol.origin[a]) / float(vol.voxel) + 0.5) for a in range(3)]
    if not (0 <= idx[0] < nx and 0 <= idx[1] < ny and 0 <= idx[2] < nz):
        return None
    i, j, k = (int(v) for v in idx)
    return float(vol.d[k, j, i]) if vol.w[k, j, i] >= min_weight else None


def tri_scalar(vol, P, min_weight):
    nx, ny, nz = vol.dims
    g = [(P[a] - vol.origin[a]) / float(vol.voxel) for a in range(3)]
    b = [np.floor(v) for v in g]
    if not (0 <= b[0] and b[0] + 1 < nx and 0 <= b[1] and b[1] + 1 < ny and 0 <= b[2] and b[2] + 1 < nz):
        return None
    f = [g[a] - b[a] for a in range(3)]
    i, j, k = (int(v) for v in b)
    if (vol.w[k:k + 2, j:j + 2, i:i + 2] < min_weight).any():
        return None
    c = lambda dx, dy, dz: float(vol.d[k + dz, j + dy, i + dx])
    lerp = lambda lo, hi, t: lo + t * (hi - lo)
    x = [[lerp(c(0, dy, dz), c(1, dy, dz), f[0]) for dy in (0, 1)] for dz in (0, 1)]
    y = [lerp(x[dz][0], x[dz][1], f[1]) for dz in (0, 1)]
    return lerp(y[0], y[1], f[2])


def raycast_pixel(vol, u, v, intr, pose, z_near, z_far, ray_step, min_weight):
    """(depth float32, interpolated) of one pixel"""
    fx, fy, ppx, ppy = (float(q) for q in intr)
    T = np.asarray(pose, F64).reshape(4, 4).tolist()
    step, K = O.ray_steps(vol, z_near, z_far, ray_step)
    c = [-((T[0][a] * T[0][3] + T[1][a] * T[1][3]) + T[2][a] * T[2][3]) for a in range(3)]
    dc = [(float(u) - ppx) / fx, (float(v) - ppy) / fy, 1.0]
    dw = [(T[0][a] * dc[0] + T[1][a] * dc[1]) + T[2][a] * dc[2] for a in range(3)]
    point = lambda s: [c[a] + s * dw[a] for a in range(3)]
    zn = float(F32(z_near))
    prev = None
    for k in range(K):
        cur = near_scalar(vol, point(zn + float(k) * step), min_weight)
        if cur is not None and not cur > 0:
            if k >= 1 and prev is not None:   # prev is a front sample: a back one would have ended the walk
                s0, s1 = zn + float(k - 1) * step, zn + float(k) * step
                a0, a1 = tri_scalar(vol, point(s0), min_weight), tri_scalar(vol, point(s1), min_weight)
                interp = a0 is not None and a1 is not None and a0 > 0 >= a1
                f0, f1 = (a0, a1) if interp else (prev, cur)
                return F32(s0 + step * f0 / (f0 - f1)), interp
            return F32(0), False
        prev = cur
    return F32(0), False


def extract_loops(vol, min_weight):
    nx, ny, nz = vol.dims
    v = float(vol.voxel)

    def grad(i, j, k):
        if not (1 <= i < nx - 1 and 1 <= j < ny - 1 and 1 <= k < nz - 1):
            return None
        nb = [(k, j, i + 1), (k, j, i - 1), (k, j + 1, i), (k, j - 1, i), (k + 1, j, i), (k - 1, j, i)]
        if any(vol.w[q] < min_weight for q in nb):
            return None
        return [float(vol.d[nb[2 * a]]) - float(vol.d[nb[2 * a + 1]]) for a in range(3)]

    rows, n_cross = [], 0
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for a in range(3):
                    m = (i + (a == 0), j + (a == 1), k + (a == 2))
                    if m[0] >= nx or m[1] >= ny or m[2] >= nz:
                        continue
                    if vol.w[k, j, i] < min_weight or vol.w[m[2], m[1], m[0]] < min_weight:
                        continue
                    d0, d1 = float(vol.d[k, j, i]), float(vol.d[m[2], m[1], m[0]])
                    if not (abs(d0) < 1 and abs(d1) < 1) or (d0 > 0) == (d1 > 0):
                        continue
                    n_cross += 1
                    g0, g1 = grad(i, j, k), grad(*m)
                    if g0 is None or g1 is None:
                        continue
                    t = d0 / (d0 - d1)
                    g = [g0[b] + t * (g1[b] - g0[b]) for b in range(3)]
                    ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
                    if not ln > 0:
                        continue
                    P = [vol.origin[0] + float(i) * v, vol.origin[1] + float(j) * v, vol.origin[2] + float(k) * v]
                    P[a] = P[a] + t * v
                    rows.append([F32(q) for q in P] + [F32(q / ln) for q in g])
    return np.array(rows, F32).reshape(-1, 6), n_cross


TINY_INTR = (60.0, 55.0, 11.5, 9.5)


def tiny_image(seed):
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.55, 0.75, (20, 24)).astype(F32)
    return cases.spoiled(img, seed)


def tiny_pose(seed):
    return cases.true_motion(seed, 15.0, 4.0)


@pytest.mark.parametrize("seed", range(3))
def test_integrate_equals_the_loops(seed):
    a, b = tiny_volume(seed), tiny_volume(seed)
    for f in range(3):
        img, pose = tiny_image(10 * seed + f), tiny_pose(seed + f)
        na = O.integrate(a, img, TINY_INTR, pose, z_min=0.5)
        nb = integrate_loops(b, img, TINY_INTR, pose, z_min=0.5)
        assert na == nb and na > 0
        assert a.records().tobytes() == b.records().tobytes()
    # a z range that cuts through the images' 0.55 .. 0.75 m: fewer voxels than without it, z_min and z_max each their own
    img = tiny_image(seed)
    counts = []
    for kw in (dict(), dict(z_min=0.65), dict(z_max=0.65), dict(z_min=0.62, z_max=0.68)):
        c, d = tiny_volume(seed), tiny_volume(seed)
        counts.append(O.integrate(c, img, TINY_INTR, np.eye(4), **kw))
        assert counts[-1] == integrate_loops(d, img, TINY_INTR, np.eye(4), **kw) and c.records().tobytes() == d.records().tobytes()
    assert counts[0] > max(counts[1:]) and min(counts[1:]) > 0 and counts[1] + counts[2] == counts[0]
    u16 = cases.to_u16(np.nan_to_num(tiny_image(seed), nan=0.0, posinf=0.0, neginf=0.0).clip(0, 60))
    assert O.integrate(a, u16, TINY_INTR, np.eye(4)) == integrate_loops(b, u16, TINY_INTR, np.eye(4))
    assert a.records().tobytes() == b.records().tobytes()


@pytest.mark.parametrize("min_weight", [1, 2])
def test_near_and_tri_equal_the_scalars(min_weight):
    vol = tiny_volume(3, observed=0.97)
    vol.w[vol.w == 1] = 3     # most cells of eight pass min_weight 2 ...
    vol.w[1, 2, 3] = 1        # ... and this voxel does not
    rng = np.random.default_rng(4)
    lo = np.array(vol.origin) - 0.03
    hi = np.array(vol.origin) + np.array(vol.dims) * float(vol.voxel) + 0.01
    pts = rng.uniform(lo, hi, (400, 3))
    pts[:8] = np.array(vol.origin) + np.array([[0, 0, 0], [4, 3, 2], [0.5, 0.5, 0.5], [-0.5, 0, 0], [4.5, 3, 2], [3.999, 2.999, 1.999],
                                               [4, 0, 0], [0, 3, 0]]) * float(vol.voxel)
    P = [pts[:, a].copy() for a in range(3)]
    ok_n, d_n = O.near(vol, P, min_weight)
    ok_t, d_t = O.tri(vol, P, min_weight)
    for q in range(len(pts)):
        want = near_scalar(vol, pts[q], min_weight)
        assert (want is not None) == bool(ok_n[q]) and (want is None or F64(want).tobytes() == d_n[q].tobytes())
        want = tri_scalar(vol, pts[q], min_weight)
        assert (want is not None) == bool(ok_t[q]) and (want is None or F64(want).tobytes() == d_t[q].tobytes())
    assert ok_n.any() and not ok_n.all() and ok_t.any() and not ok_t.all()


@pytest.mark.parametrize("ray_step,min_weight,z_near", [(0.5, 1, 0.5), (1.0, 1, 0.49), (0.25, 2, 0.5)])
def test_the_walk_equals_the_per_pixel_loop(ray_step, min_weight, z_near):
    vol = O.Volume((5, 4, 3), 0.02, (-0.04, -0.03, 0.60), trunc=0.05, max_weight=3)
    rng = np.random.default_rng(5)
    for f in range(3):   # a real surface, so that rays bracket it; the third frame leaves some voxels at weight 1
        O.integrate(vol, rng.uniform(0.60, 0.66, (20, 24)).astype(F32), TINY_INTR, tiny_pose(f) if f else np.eye(4))
    pose = cases.true_motion(8, 5.0, 2.0)
    depth, _, st = O.raycast(vol, (9, 11), (70.0, 70.0, 5.0, 4.0), pose, z_near=z_near, z_far=0.8, ray_step=ray_step, min_weight=min_weight)
    n_hit = n_int = 0
    for v in range(9):
        for u in range(11):
            want, interp = raycast_pixel(vol, u, v, (70.0, 70.0, 5.0, 4.0), pose, z_near, 0.8, ray_step, min_weight)
            assert want.tobytes() == depth[v, u].tobytes(), (u, v)
            n_hit += want > 0
            n_int += interp
    assert (st["n_hits"], st["n_interpolated"]) == (n_hit, n_int) and n_hit > 0


@pytest.mark.parametrize("seed,min_weight", [(0, 1), (1, 1), (2, 2)])
def test_extraction_order_equals_the_loops(seed, min_weight):
    vol = tiny_volume(seed, observed=1.0)
    if min_weight == 2:
        vol.w[vol.w == 1] = 2
        vol.w[0, 0, 0] = vol.w[1, 1, 4] = 1   # a corner, and a neighbour of the last interior voxel
    rows, st = O.extract(vol, min_weight)
    want, n_cross = extract_loops(vol, min_weight)
    assert st["n_crossings"] == n_cross and st["n_rows"] == len(want) == len(rows)
    assert rows.tobytes() == want.tobytes()
    assert n_cross > len(want) > 0   # the border's crossings have no gradient


# ---- known answers ---------------------------------------------------------------------------------------------------
def test_an_empty_volume_gives_nothing():
    vol = O.Volume(**VC.SPHERE_VOLUME)
    depth, normals, st = O.raycast(vol, (30, 40), cases.intrinsics(30, 40), np.eye(4), normals=True, **VC.SPHERE_RAYCAST)
    assert not depth.any() and not normals.any() and st["n_hits"] == 0
    rows, st = O.extract(vol)
    assert rows.shape == (0, 6) and st["n_crossings"] == st["n_rows"] == 0


def test_weight_cap_reset_and_untouched_voxels():
    vol = O.Volume((5, 4, 3), 0.02, (-0.04, -0.03, 0.60), trunc=0.05, max_weight=3)
    imgs = [np.full((20, 24), 0.63 + 0.002 * f, F32) for f in range(5)]
    for img in imgs:
        img[:, 12:] = 0.0                          # half the image is a hole
        before = vol.records().copy()
        n = O.integrate(vol, img, TINY_INTR, np.eye(4))
        assert before.tobytes() != vol.records().tobytes() and 0 < n < vol.d.size
    assert set(np.unique(vol.w)) == {0, 3}
    # the capped recurrence for a voxel near the optical axis, which sees every frame's z
    i, j, k = 2, 1, 0
    assert vol.w[k, j, i] == 3
    p2 = vol.origin[2] + float(k) * float(vol.voxel)
    d, w = F32(1), 0
    for img in imgs:
        dn = min((float(img[0, 0]) - p2) / float(vol.trunc), 1.0)
        d = F32((float(d) * float(w) + dn) / float(w + 1))
        w = min(w + 1, 3)
    img = imgs[0]
    assert vol.w[k, j, i] == 3 and vol.d[k, j, i].tobytes() == d.tobytes()
    # a voxel outside the image or behind the camera keeps its bytes
    back = np.eye(4)
    back[2, 3] = -2.0                              # the whole volume behind the camera
    before = vol.records().copy()
    assert O.integrate(vol, img, TINY_INTR, back) == 0 and before.tobytes() == vol.records().tobytes()
    side = np.eye(4)
    side[0, 3] = 5.0                               # and far outside the image
    assert O.integrate(vol, img, TINY_INTR, side) == 0 and before.tobytes() == vol.records().tobytes()
    vol.reset()
    assert (vol.d == F32(1)).all() and not vol.w.any() and vol.integrations == 0


def test_the_volume_does_not_depend_on_how_a_stream_is_split():
    frames, poses = cases.stream(4, 3, 20.0, 2.0, 30, 40)
    intr = cases.intrinsics(30, 40)
    a, b = O.Volume(**VC.small_volume((12, 11, 10))), O.Volume(**VC.small_volume((12, 11, 10)))
    for f, P in zip(frames, poses):
        O.integrate(a, f, intr, P)
    for f, P in zip(frames[:2], poses[:2]):
        O.integrate(b, f, intr, P)
    mid = b.records().copy()
    b.d, b.w = mid["d"].reshape(b.d.shape).copy(), mid["w"].reshape(b.w.shape).copy()   # as read back and continued
    for f, P in zip(frames[2:], poses[2:]):
        O.integrate(b, f, intr, P)
    assert a.records().tobytes() == b.records().tobytes() and a.w.max() == 4


# ---- accuracy: every bound is twice what the oracle measured (the module's docstring) ---------------------------------
@pytest.fixture(scope="module")
def scene():
    frames, poses = cases.stream(4, 3, 20.0, 2.0)
    vol = O.Volume(**VC.SCENE_VOLUME)
    for f, P in zip(frames, poses):
        O.integrate(vol, f, INTR, P)
    return vol, frames, poses


def test_one_frame_comes_back(scene):
    _, frames, _ = scene
    vol = O.Volume(**VC.SCENE_VOLUME)
    O.integrate(vol, frames[0], INTR, np.eye(4))
    depth = O.raycast(vol, VC.SHAPE, INTR, np.eye(4), **VC.SCENE_RAYCAST)[0]
    rms, worst, median, share = VC.compare(depth, frames[0])
    print(f"round trip: rms {rms * 1e3:.2f} mm, worst {worst * 1e3:.1f} mm, median {median * 1e3:.2f} mm, share {share:.4f}")
    assert median <= 2 * 0.0025 and rms <= 2 * 0.0342 and worst <= 2 * 0.392 and share >= 1 - 2 * (1 - 0.879)


def test_raycast_accuracy_on_the_analytic_scene(scene):
    vol, _, poses = scene
    unseen = cases.true_motion(99, 25.0, 2.5) @ poses[1]
    for name, P, rms_max, share_min in [("seen", P, 0.0306, 0.928) for P in poses] + [("unseen", unseen, 0.0258, 0.928)]:
        depth = O.raycast(vol, VC.SHAPE, INTR, P, **VC.SCENE_RAYCAST)[0]
        rms, worst, median, share = VC.compare(depth, cases.render(P))
        print(f"{name}: rms {rms * 1e3:.2f} mm, worst {worst * 1e3:.1f} mm, median {median * 1e3:.2f} mm, share {share:.4f}")
        assert rms <= 2 * rms_max and median <= 2 * 0.00056 and share >= 1 - 2 * (1 - share_min)


def test_sphere_raycast_and_extraction():
    vol = O.Volume(**VC.SPHERE_VOLUME)
    for f, T in zip(VC.sphere_frames(), VC.SPHERE_VIEWS):
        O.integrate(vol, f, INTR, T)
    for f, T in zip(VC.sphere_frames(), VC.SPHERE_VIEWS):
        depth = O.raycast(vol, VC.SHAPE, INTR, T, **VC.SPHERE_RAYCAST)[0]
        rms, worst, median, share = VC.compare(depth, f)
        extra = int(((depth > 0) & ~(f > 0)).sum()) / float((f > 0).sum())
        print(f"sphere view: rms {rms * 1e3:.2f} mm, worst {worst * 1e3:.1f} mm, share {share:.4f}, extra {extra:.4f}")
        assert rms <= 2 * 0.0035 and share >= 1 - 2 * (1 - 0.991) and extra <= 2 * 0.037
    rows, st = O.extract(vol)
    off = np.linalg.norm(rows[:, :3].astype(F64) - VC.SPHERE_C, axis=1)
    r = off - VC.SPHERE_R
    dots = (rows[:, 3:].astype(F64) * (rows[:, :3].astype(F64) - VC.SPHERE_C) / off[:, None]).sum(1)
    print(f"extract: {st}, rms {np.sqrt((r * r).mean()) * 1e3:.3f} mm, worst {np.abs(r).max() * 1e3:.2f} mm, min dot {dots.min():.3f}")
    assert st["n_rows"] == len(rows) > 3000
    assert np.sqrt((r * r).mean()) <= 2 * 0.00072 and np.abs(r).max() <= 2 * 0.0048 and dots.min() >= 1 - 2 * (1 - 0.81)
    assert np.abs(np.linalg.norm(rows[:, 3:].astype(F64), axis=1) - 1).max() < 1e-6


def test_fused_chain_against_the_frame_to_frame_chain():
    frames, poses = cases.stream(4, 5, 20.0, 2.0)
    fus = O.Fusion(VC.SHAPE, INTR, O.Volume(**VC.SCENE_VOLUME), raycast_params=VC.SCENE_RAYCAST)
    chain = np.eye(4)
    for i, f in enumerate(frames):
        T, status = fus.push(f)
        assert status == (MO.NONE if i == 0 else MO.CONVERGED)
        if i:
            chain = O.mat44_mul(MO.motion(frames[i - 1], f, INTR)[0], chain)
    fused, odo = MO.pose_error(fus.pose, poses[-1]), MO.pose_error(chain, poses[-1])
    print(f"fused chain {fused[0]:.3f} mm {fused[1]:.4f} deg; frame-to-frame chain {odo[0]:.3f} mm {odo[1]:.4f} deg; "
          f"ratio {fused[0] / odo[0]:.2f} / {fused[1] / odo[1]:.2f}")
    assert fused[0] <= 2 * 0.86 and fused[1] <= 2 * 0.019
    assert fus.vol.integrations == 4 and fus.model_depth.shape == VC.SHAPE
