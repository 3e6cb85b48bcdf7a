"""Hand-made inputs for ppf_refine_frame that the CPU tests of tests/refine_oracle.py (tests/test_refine_cases.py) and the
device tests (tests/test_gpu_refine.py) share: image edges, depth holes, rows behind the camera, non-finite rows and poses,
the guards at equality, a singular system, the sizes at which the kernel's sums change tile, unequal and negative focal lengths.

case(name) is a dict: `name`; `pins`, the rules of refine_oracle.MUTANTS the case is there to pin (by rule name; empty for a
case that only has to come through); `runs`, one per call of ppf_refine_frame.  A run is a dict: `what`, `models` (a list of
(n, 6) float32), `poses` (per model, a list of 4 x 4 starts), `depth`, `intr`, `prm` (what differs from the defaults) and
`hand`: {(model, pose): {info field: value}}, counts worked out by hand, not by the oracle.  Further keys of a case hold
what its condition in tests/test_refine_cases.py needs."""
import functools

import numpy as np

import refine_oracle as R
import render_oracle as RO

F32 = np.float32
ROWS, COLS = 120, 160
INTR = (300.0, 300.0, 79.5, 59.5)
NAMES = ("lattice", "near_zero", "gate_edge", "holes", "borders", "shell", "bad_rows", "guards", "plane", "sizes", "limits",
         "intrinsics")


def draw(model, T, background, rows=ROWS, cols=COLS, intr=INTR, radius=0.003):
    """the z-buffer of the posed model at `radius` splats, `background` where nothing is drawn"""
    zb = RO.zbuffer(R.transform_rows(model, T), rows, cols, intr, radius)
    depth = zb.view(F32).copy()
    depth[zb == RO.EMPTY32] = background
    return depth


def true_pose():
    T = np.eye(4)
    T[:3, :3] = R.rot_vec([0.4, -0.3, 0.2])
    T[:3, 3] = [0.01, -0.005, 0.6]
    return T


def start(T, seed, mm, deg):
    """T moved by (mm, deg) in the random directions of `seed`, the rotation about T's translation; T itself for (0, 0)"""
    if not mm and not deg:
        return T.copy()
    t, r = R.random_offset(np.random.default_rng(seed), mm, deg)
    return R.offset_pose(T, T[:3, 3].copy(), t, r)


def run(what, models, poses, depth, intr=INTR, prm=None, hand=None):
    return dict(what=what, models=[np.ascontiguousarray(m, dtype=F32) for m in models], poses=poses,
                depth=np.ascontiguousarray(depth, dtype=F32), intr=tuple(float(v) for v in intr), prm=dict(prm or {}), hand=dict(hand or {}))


@functools.lru_cache(maxsize=None)
def dense():
    """the 38,209-row ellipsoid: one row more than the 597 chunks of the c0 sum's LDS tile hold"""
    return R.ellipsoid(38209, seed=1)


@functools.lru_cache(maxsize=None)
def ellipsoid3001():
    return R.ellipsoid(3001, seed=3008)


@functools.lru_cache(maxsize=None)
def image(background):
    """the dense ellipsoid at the true pose"""
    return draw(dense(), true_pose(), background)


def plane64():
    """8 x 8 rows 10 mm apart on z = 1, facing the camera; at INTR row i lies on pixel (80 + 3 (i % 8 - 4), 60 + 3 (i / 8 - 4))"""
    i = np.arange(64)
    m = np.zeros((64, 6), F32)
    m[:, 0], m[:, 1], m[:, 2], m[:, 5] = (i % 8 - 4) * 0.01, (i // 8 - 4) * 0.01, 1, -1
    return m


def plane64_pixels():
    """(v, u) of plane64's rows at the identity pose and INTR, in plain arithmetic"""
    m = plane64()
    return [int(np.floor(float(y) * 300.0 / 1.0 + 59.5 + 0.5)) for y in m[:, 1]], [int(np.floor(float(x) * 300.0 / 1.0 + 79.5 + 0.5)) for x in m[:, 0]]


# ---- the cases ------------------------------------------------------------------------------------------------------------------
LATTICE_U = np.arange(-3, 34) * 0.5   # -1.5, -1.0, ..., 16.5: pixel coordinates on integers and half-integers


def lattice_pairs(rows, cols, checker, rounding=lambda x: int(np.floor(x + 0.5))):
    """the pairs of the lattice by integer arithmetic on (u, v): a row pairs when its pixel is in the image and not zero"""
    n = 0
    for v in LATTICE_U:
        for u in LATTICE_U:
            ui, vi = rounding(float(u)), rounding(float(v))
            n += 0 <= ui < cols and 0 <= vi < rows and (not checker or (ui + vi) % 2 == 0)
    return n


def _lattice():
    intr = (256.0, 256.0, 8.0, 8.0)
    uu, vv = np.meshgrid(LATTICE_U, LATTICE_U)
    m = np.zeros((uu.size, 6), F32)
    m[:, 0], m[:, 1], m[:, 2], m[:, 5] = (uu.ravel() - 8) / 256, (vv.ravel() - 8) / 256, 1, -1   # exact in fp32
    runs = []
    for rows in (16, 11):
        for checker in (False, True):
            d = np.ones((rows, 16), F32)
            if checker:
                V, U = np.mgrid[0:rows, 0:16]
                d[(U + V) % 2 == 1] = 0
            n = lattice_pairs(rows, 16, checker)
            runs.append(run(f"{rows} x 16 {'checkerboard' if checker else 'ones'}", [m], [[np.eye(4)]], d, intr,
                            dict(min_pair_share=0.0) if checker else {},
                            {(0, 0): dict(status=R.CONVERGED, iterations=1, n_rows=1369, n_considered=1369, n_pairs_first=n, n_pairs_last=n)}))
    return dict(pins=("rounding",), runs=runs)


def _near_zero():
    g = np.arange(8) - 3.5
    xx, yy = np.meshgrid(g, g)
    front = np.zeros((64, 6), F32)
    front[:, 0], front[:, 1], front[:, 2], front[:, 5] = xx.ravel() * 0.01 / 300 * 4, yy.ravel() * 0.01 / 300 * 4, 0.01, -1   # 4 pixels apart
    back = front.copy()
    back[:, 2], back[:, 5] = -0.005, 1      # faces the camera from behind it
    tang = np.zeros((64, 6), F32)
    tang[:, 2], tang[:, 3] = 1, 1           # (0, 0, 1) with normal (1, 0, 0): facing == 0
    m = np.concatenate([front, back, tang])
    prm = dict(min_pair_share=0.0)
    runs = [run("constant 0.01", [m], [[np.eye(4)]], np.full((ROWS, COLS), 0.01, F32), INTR, prm,
                {(0, 0): dict(n_rows=192, n_considered=128, n_pairs_first=64)}),
            run("all zero", [m], [[np.eye(4)]], np.zeros((ROWS, COLS), F32), INTR, prm,
                {(0, 0): dict(status=R.LOST, iterations=0, n_rows=192, n_considered=128, n_pairs_first=0, n_pairs_last=0)})]
    return dict(pins=("d_positive", "z_positive", "facing"), runs=runs)


def _gate_edge():
    gate = F32(2.0 ** -6)
    d = np.full((ROWS, COLS), F32(1) + gate, F32)   # d - z == gate exactly
    runs = [run("gate 2^-6", [plane64()], [[np.eye(4)]], d, INTR, dict(depth_gate=float(gate)), {(0, 0): dict(n_considered=64, n_pairs_first=64)}),
            run("gate below 2^-6", [plane64()], [[np.eye(4)]], d, INTR, dict(depth_gate=float(np.nextafter(gate, F32(0)))),
                {(0, 0): dict(status=R.LOST, iterations=0, n_considered=64, n_pairs_first=0, n_pairs_last=0)})]
    return dict(pins=("gate",), runs=runs)


HOLE_VALUES = np.array([0.0, np.nan, np.inf, -0.6, -np.inf], F32)


def punch(depth, share, seed):
    """a copy of depth with a seeded `share` of its pixels > 0 overwritten by HOLE_VALUES"""
    rng = np.random.default_rng(seed)
    out = depth.copy()
    obj = np.argwhere(np.isfinite(depth) & (depth > 0))
    pick = obj[rng.choice(len(obj), int(len(obj) * share), replace=False)]
    out[pick[:, 0], pick[:, 1]] = HOLE_VALUES[rng.integers(0, len(HOLE_VALUES), len(pick))]
    return out


def _holes():
    T = true_pose()
    whole = image(0.0)
    poses = [start(T, k, mm, deg) for k, (mm, deg) in enumerate(((0, 0), (2, 1), (5, 3), (10, 5)))]
    return dict(pins=(), whole=whole, runs=[run("a fifth of the object's pixels", [ellipsoid3001()], [poses], punch(whole, 0.2, 5))])


def _borders():
    runs = []
    for what, (tx, ty) in dict(left=(-0.155, 0.0), right=(0.16, 0.0), top=(0.0, -0.118), bottom=(0.0, 0.12), corner=(0.15, 0.11)).items():
        Tb = true_pose()
        Tb[0, 3], Tb[1, 3] = tx, ty
        runs.append(run(what, [ellipsoid3001()], [[start(Tb, 9, 2, 1)]], draw(dense(), Tb, 0.9)))
    return dict(pins=("rounding",), runs=runs)


def _shell():
    intr = (100.0, 100.0, 79.5, 59.5)
    axes = (0.3, 0.25, 0.4)
    shell = R.ellipsoid(3001, axes=axes, seed=11)
    drawn = R.ellipsoid(60000, axes=axes, seed=12)
    shell[:, 3:] *= -1   # inward normals: the camera is inside
    drawn[:, 3:] *= -1
    Ts = np.eye(4)
    Ts[:3, :3] = R.rot_vec([0.1, 0.2, -0.1])
    Ts[:3, 3] = [0.02, -0.01, 0.05]
    o = R.transform_rows(drawn, Ts)
    zb = RO.zbuffer(o[o[:, 2] > 0.01], ROWS, COLS, intr, 0.01)
    d = zb.view(F32).copy()
    d[zb == RO.EMPTY32] = 0
    poses = [start(Ts, k, mm, deg) for k, (mm, deg) in enumerate(((0, 0), (5, 1), (10, 2)))]
    return dict(pins=("share",), T=Ts, runs=[run("share 0.1", [shell], [poses], d, intr, dict(min_pair_share=0.1)),
                                            run("default share", [shell], [poses], d, intr)])


def _bad_rows():
    T0 = start(true_pose(), 1, 5, 3)
    clean = ellipsoid3001()
    bad = clean.copy()
    idx = np.random.default_rng(3).choice(3001, 300, replace=False)
    bad[idx[:100], 0] = np.nan
    bad[idx[100:200], 4] = np.inf
    bad[idx[200:], 2] = -np.inf
    nan_pose, inf_pose = T0.copy(), T0.copy()
    nan_pose[1, 2] = np.nan
    inf_pose[0, 3] = np.inf
    nothing = dict(status=R.LOST, iterations=0, n_considered=0, n_pairs_first=0, n_pairs_last=0)
    return dict(pins=("c0",), clean=clean, bad=bad,
                runs=[run("300 spoiled rows; 130 NaN rows; a NaN pose, an inf translation", [bad, np.full((130, 6), np.nan, F32), clean],
                          [[T0], [T0], [nan_pose, inf_pose]], image(0.9), INTR, {},
                          {(1, 0): dict(nothing, n_rows=130), (2, 0): dict(nothing, n_rows=3001), (2, 1): dict(nothing, n_rows=3001)})])


def _guards():
    ones = np.ones((ROWS, COLS), F32)
    half = ones.copy()
    v, u = plane64_pixels()
    half[v[32:], u[32:]] = 0   # rows 32..63 lose their pixel
    went = dict(status=R.CONVERGED, iterations=1, n_considered=64)
    lost = dict(status=R.LOST, iterations=0, n_considered=64)
    above = float(np.nextafter(F32(0.5), F32(1)))
    runs = [run("min_pairs 64", [plane64()], [[np.eye(4)]], ones, INTR, dict(min_pairs=64, min_pair_share=0.0), {(0, 0): dict(went, n_pairs_first=64, n_pairs_last=64)}),
            run("min_pairs 65", [plane64()], [[np.eye(4)]], ones, INTR, dict(min_pairs=65, min_pair_share=0.0), {(0, 0): dict(lost, n_pairs_first=64, n_pairs_last=64)}),
            run("share 0.5", [plane64()], [[np.eye(4)]], half, INTR, dict(min_pairs=6, min_pair_share=0.5), {(0, 0): dict(went, n_pairs_first=32, n_pairs_last=32)}),
            run("share above 0.5", [plane64()], [[np.eye(4)]], half, INTR, dict(min_pairs=6, min_pair_share=above), {(0, 0): dict(lost, n_pairs_first=32, n_pairs_last=32)})]
    return dict(pins=("min_pairs", "share"), runs=runs)


def _plane():
    g = (np.arange(17) - 8) * 0.004
    xx, yy = np.meshgrid(g, g)
    pl = np.zeros((289, 6), F32)
    pl[:, 0], pl[:, 1], pl[:, 5] = xx.ravel(), yy.ravel(), -1
    Tp = np.eye(4)
    Tp[2, 3] = 0.5
    deeper = Tp.copy()
    deeper[2, 3] = 0.504
    tilted = R.offset_pose(Tp, Tp[:3, 3].copy(), [0.001, 0.002, 0.003], [0.02, -0.01, 0.03])
    d = np.full((ROWS, COLS), 0.5, F32)
    # the same lattice with every normal (1, 2, -2) / 3 on an image 1 mm behind it.  n1 == -n2 in every row, so every sum with n1 is
    # the negative of the sum with n2, bit for bit, and stays so through the elimination of columns 0..2; in column 3 the
    # candidates are sum n0 n0 + lambda < |sum n1 n0| == |sum n2 n0|: rows 4 and 5 tie for the pivot
    # The two choices differ in the last bit of t1 and t2 (about 4e-4), so the pose is the identity and the model itself lies at
    # z = 0.5: the difference then lands in T[1][3], next to 0, and not next to a translation of 0.5 whose rounding would swallow it.
    # One step only: the next evaluation rounds the moved rows to fp32 and both choices meet again.
    tied = pl.copy()
    tied[:, 2] = 0.5
    tied[:, 3:] = np.array([1, 2, -2], np.float64) / 3
    runs = [run("exact, 4 mm deeper, tilted", [pl], [[Tp, deeper, tilted]], d),
            run("tilted, eps 0, 100 iterations", [pl], [[tilted]], d, INTR, dict(eps_rot=0.0, eps_trans=0.0, max_iters=100)),
            run("tied pivots, one step", [tied], [[np.eye(4)]], np.full((ROWS, COLS), 0.501, F32), INTR, dict(max_iters=1))]
    return dict(pins=("pivot",), iterations=(1, 2, 3), runs=runs)


def _sizes():
    T = true_pose()
    models = [R.ellipsoid(n, seed=n) for n in (4096, 4097, 38209)]   # 64 and 65 chunks; one row more than 597 chunks
    poses = [[start(T, n, 5, 3)] for n in (4096, 4097, 38209)]
    p64 = plane64()
    prm = dict(min_pairs=6, min_pair_share=0.0)
    cuts = [p64[:n] for n in (1, 6, 15, 16, 63, 64)] + [np.concatenate([p64, p64[:1]])]
    m128 = R.ellipsoid(128, seed=135)
    ones = np.ones((ROWS, COLS), F32)
    # the plane moved onto the background at 0.9, to the right of and below the object.  The jobs after the large one start
    # 597 chunks further into the partials; with the default min_pairs the 6 rows are LOST and the 16 go on
    aside = np.eye(4)
    aside[:3, 3] = [0.2, 0.1, -0.1]
    runs = [run("4,096, 4,097 and 38,209 rows, then 6 and 16", models + [p64[:6], p64[:16]], poses + [[aside], [aside]], image(0.9), INTR, {},
                {(3, 0): dict(status=R.LOST, iterations=0, n_rows=6, n_considered=6, n_pairs_first=6),
                 (4, 0): dict(status=R.CONVERGED, iterations=1, n_rows=16, n_considered=16, n_pairs_first=16)}),
            run("38,209 rows, model_step 9", [dense()], [poses[2]], image(0.9), INTR, dict(model_step=9)),
            run("1, 6, 15, 16, 63, 64 and 65 rows", cuts, [[np.eye(4)]] * len(cuts), ones, INTR, prm,
                {(0, 0): dict(status=R.LOST, iterations=0, n_rows=1, n_considered=1, n_pairs_first=1),
                 **{(i, 0): dict(status=R.CONVERGED, iterations=1, n_rows=n, n_considered=n, n_pairs_first=n) for i, n in ((1, 6), (2, 15), (3, 16), (4, 63), (5, 64), (6, 65))}}),
            run("128 rows, eps 0, 100 iterations", [m128], [[start(T, 1, 5, 3)]], image(0.9), INTR, dict(eps_rot=0.0, eps_trans=0.0, max_iters=100))]
    return dict(pins=("chunk_order",), iterations=(8, 6, 7), runs=runs)


def _limits():
    return dict(pins=(), runs=[run("max_step_rot 0.001", [ellipsoid3001()], [[start(true_pose(), 1, 5, 3)]], image(0.9), INTR, dict(max_step_rot=0.001))])


def _intrinsics():
    T = true_pose()
    T0 = start(T, 1, 5, 3)
    odd = (310.5, 295.25, 61.3, 47.9)
    flipped = draw(dense(), T, 0.0, intr=(310.5, 295.25, 81.3, ROWS - 1 - 57.9))[::-1].copy()   # row v of it is row ROWS - 1 - v as fy > 0 sees it
    return dict(pins=(), runs=[run("fx != fy on 97 x 131", [ellipsoid3001()], [[T0]], draw(dense(), T, 0.0, rows=97, cols=131, intr=odd), odd),
                               run("fy < 0", [ellipsoid3001()], [[T0]], flipped, (310.5, -295.25, 81.3, 57.9))])


@functools.lru_cache(maxsize=None)
def case(name):
    c = globals()["_" + name]()
    c["name"] = name
    assert set(c["pins"]) <= {rule for rule, _ in R.MUTANTS.values()}
    return c


def jobs(c):
    """(run, model index, pose index) of every pose of the case"""
    return [(r, i, k) for r in c["runs"] for i, plist in enumerate(r["poses"]) for k in range(len(plist))]


# ---- the fixture of tests/test_gpu_refine.py::case, for the record of which mutants it catches ---------------------------------
def old_fixture():
    """the models, image, poses and parameter sets of tests/test_gpu_refine.py::test_byte_parity_with_the_oracle, as runs"""
    sizes = (50, 128, 3001)
    models = [R.ellipsoid(n, seed=7 + n) for n in sizes]
    T = true_pose()
    depth = draw(models[2], T, 0.9)
    poses = []
    for i in range(3):
        starts = [T.copy()]
        for k, (mm, deg) in enumerate(((2, 1), (5, 3), (10, 5))):
            t, r = R.random_offset(np.random.default_rng(100 * i + k), mm, deg)
            starts.append(R.offset_pose(T, T[:3, 3].copy(), t, r))
        poses.append(starts)
    far = T.copy()
    far[0, 3] += 0.2
    poses[1][3] = far
    poses[0] = poses[0][:3]
    return dict(name="old fixture", pins=(), runs=[run(str(prm), models, poses, depth, INTR, prm) for prm in
                                                   (dict(model_step=1), dict(model_step=3), dict(model_step=1, max_iters=2), dict(model_step=1, max_step_trans=0.002))])


# ---- random draws (tests/test_gpu_refine.py::test_refine_random_draw) -----------------------------------------------------------
def surface(kind, n, seed):
    """n rows of an ellipsoid seen from outside, a 80 mm plane patch, or the shell seen from inside"""
    if kind == "plane":
        m = np.zeros((n, 6), F32)
        m[:, :2] = np.random.default_rng(seed).uniform(-0.04, 0.04, (n, 2))
        m[:, 5] = -1
        return m
    m = R.ellipsoid(n, axes=(0.3, 0.25, 0.4) if kind == "shell" else (0.030, 0.045, 0.070), seed=seed)
    if kind == "shell":
        m[:, 3:] *= -1
    return m


def random_draw(seed):
    """(cfg, run): one call's worth of random input; cfg is what the draw chose, for the assertion message"""
    rng = np.random.default_rng(9000 + seed)
    kind = ("ellipsoid", "plane", "shell")[int(rng.integers(0, 3))]
    n, step = int(rng.integers(1, 5001)), int(rng.integers(1, 8))
    rows, cols = 2 * int(rng.integers(10, 60)) + 1, 2 * int(rng.integers(10, 80)) + 1   # odd, up to 119 x 159
    fx = float(rng.uniform(80, 120) if kind == "shell" else rng.uniform(200, 320))
    fy = fx * float(rng.choice([-1, 1]) * rng.uniform(0.05, 0.15) + 1)                # fx != fy
    intr = (fx, fy, (cols - 1) / 2 + float(rng.uniform(-3, 3)), (rows - 1) / 2 + float(rng.uniform(-3, 3)))
    holes = float(rng.uniform(0, 0.4))
    gate = float(rng.choice([0.005, 0.01, 0.02]))
    T = np.eye(4)
    T[:3, :3] = R.rot_vec(rng.normal(size=3) * (0.1 if kind != "ellipsoid" else 1.0))
    T[:3, 3] = [0.02, -0.01, 0.05] if kind == "shell" else [float(rng.uniform(-0.02, 0.02)), float(rng.uniform(-0.02, 0.02)), float(rng.uniform(0.4, 0.7))]
    o = R.transform_rows(surface(kind, 30000, seed + 1), T)
    zb = RO.zbuffer(o[o[:, 2] > 0.01], rows, cols, intr, 0.01 if kind == "shell" else 0.003)
    depth = zb.view(F32).copy()
    depth[zb == RO.EMPTY32] = 0.0 if kind == "shell" or rng.uniform() < 0.5 else 0.9
    depth = punch(depth, holes, seed)
    starts = [(float(rng.uniform(0, 12)), float(rng.uniform(0, 6))) for _ in range(int(rng.integers(1, 5)))]
    poses = [start(T, 100 * seed + k, mm, deg) for k, (mm, deg) in enumerate(starts)]
    prm = dict(depth_gate=gate, model_step=step, min_pair_share=0.02)   # small images and holes leave few pairs: go on with them
    cfg = dict(seed=seed, kind=kind, n=n, model_step=step, image=(rows, cols), intr=intr, holes=round(holes, 3), gate=gate, starts=starts)
    return cfg, run(str(cfg), [surface(kind, n, seed)], [poses], depth, intr, prm)
