"""A numpy restatement of DESIGN.md §17: ppf_refine_frame's projective point-to-plane refinement of one pose on a depth
image.  Every step is the fp64 / fp32 arithmetic the kernel does, in the same order: products are rounded before they are
added (numpy never fuses), a chunk of 64 rows is summed by the fixed lane tree, the chunks in order, and the 6x6 solve and
the pose update are written out in scalars.  sin / cos come from the CPU checker's detmath (oracle_lib.math_eval)."""
import numpy as np

import oracle_lib

NONE, CONVERGED, MAX_ITERS, LOST, STEP = 0, 1, 2, 3, 4
CHUNK, ENTRIES = 64, 28
EPS = 1.192092896e-07
F32, F64 = np.float32, np.float64
DEFAULTS = dict(depth_gate=0.02, max_step_rot=0.35, max_step_trans=0.03, eps_rot=1e-5, eps_trans=1e-5, min_pair_share=0.25,
                min_pairs=16, max_iters=20, model_step=1)
INFO_FIELDS = ["status", "iterations", "n_rows", "n_considered", "n_pairs_first", "n_pairs_last", "rmse_first", "rmse_last"]
# One altered rule at a time, for tests/test_refine_cases.py: `mutant` below is None (the specification) or one of these names;
# the value is (the rule it alters, by the name the cases of tests/refine_cases.py pin it under, what it does instead).
# No mutant reads a pixel outside the image: the bounds test on (ui, vi) is never altered.
MUTANTS = {
    "round_half_even": ("rounding", "pixel rounding: half to even in place of floor(x + 0.5)"),
    "round_truncate": ("rounding", "pixel rounding: x + 0.5 truncated toward zero in place of floor(x + 0.5)"),
    "gate_strict": ("gate", "|d - z| < gate in place of <="),
    "no_d_positive": ("d_positive", "d > 0 dropped"),
    "no_z_positive": ("z_positive", "z > 0 dropped"),
    "facing_le": ("facing", "facing <= 0 in place of < 0"),
    "min_pairs_le": ("min_pairs", "n_pairs <= min_pairs in place of <"),
    "share_le": ("share", "n_pairs <= share * n_considered in place of <"),
    "c0_over_rows": ("c0", "c0 divided by n_rows in place of the number of finite rows"),
    "c0_all_rows": ("c0", "c0 over all rows, non-finite values replaced by 0 and still counted"),
    "chunks_reversed": ("chunk_order", "chunk partials added in reverse order"),
    "pivot_last": ("pivot", "the last largest pivot in place of the first"),
}


def params(**kw):
    return dict(DEFAULTS, **kw)


def transform_rows(rows, T):
    """icp_transform_row on every row: the moved rows as float32 (n, 6)"""
    T = np.asarray(T, dtype=F64).reshape(4, 4)
    p = rows[:, :3].astype(F64)
    n = rows[:, 3:6].astype(F64)
    with np.errstate(all="ignore"):
        v = [((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(4)]
        div = np.abs(v[3]) > EPS
        xyz = [np.where(div, v[k] / v[3], v[k]) for k in range(3)]
        nn = [(T[r, 0] * n[:, 0] + T[r, 1] * n[:, 1]) + T[r, 2] * n[:, 2] for r in range(3)]
        nrm = np.sqrt((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2])
        big = nrm > EPS
        nn = [np.where(big, nn[k] / nrm, nn[k]) for k in range(3)]
        return np.stack(xyz + nn, axis=1).astype(F32)


def chunk_sums(vals, mutant=None):
    """vals (n, m) float64, row j = what lane j % 64 of chunk j // 64 holds: the (m,) sums by the lane tree, chunks in order"""
    n, m = vals.shape
    nc = (n + CHUNK - 1) // CHUNK
    v = np.zeros((nc * CHUNK, m), dtype=F64)   # the lanes past the last row hold +0.0
    v[:n] = vals
    v = v.reshape(nc, CHUNK, m)
    with np.errstate(all="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            v = v[:, :off] + v[:, off:2 * off]
        acc = np.zeros(m, dtype=F64)
        for c in (range(nc - 1, -1, -1) if mutant == "chunks_reversed" else range(nc)):
            acc = acc + v[c, 0]
    return acc


def chunk_sums_loop(vals):
    """the same sums by a plain loop over chunks and lanes (what tests/test_refine_oracle.py holds chunk_sums against)"""
    n, m = vals.shape
    out = []
    for e in range(m):
        acc = 0.0
        for c0 in range(0, n, CHUNK):
            lanes = [float(vals[c0 + l, e]) if c0 + l < n else 0.0 for l in range(CHUNK)]
            for off in (32, 16, 8, 4, 2, 1):
                for l in range(off):
                    lanes[l] = lanes[l] + lanes[l + off]
            acc = acc + lanes[0]
        out.append(acc)
    return np.array(out, dtype=F64)


def centre(model, step, mutant=None):
    """c0: the mean of the finite scored model rows' xyz"""
    rows = model[::step]
    fin = np.isfinite(rows[:, :6]).all(axis=1)
    vals = np.where(fin[:, None], rows[:, :3].astype(F64), 0.0)
    n = int(fin.sum())
    if mutant == "c0_over_rows":
        n = len(rows)
    if mutant == "c0_all_rows":
        vals, n = np.where(np.isfinite(rows[:, :3]), rows[:, :3].astype(F64), 0.0), len(rows)
    s = chunk_sums(vals, mutant)
    return s / F64(n) if n else np.zeros(3)


def evaluate(rows, T, c0, depth, intr, gate, mutant=None):
    """one evaluation: (the 28 sums, n_considered, n_pairs, c_k)"""
    fx, fy, ppx, ppy = (float(v) for v in intr)
    T = np.asarray(T, dtype=F64).reshape(4, 4)
    o = transform_rows(rows, T)
    ck = np.array([((T[r, 0] * c0[0] + T[r, 1] * c0[1]) + T[r, 2] * c0[2]) + T[r, 3] for r in range(3)], dtype=F64)
    with np.errstate(all="ignore"):
        x, y, z, nx, ny, nz = (o[:, k].astype(F64) for k in range(6))
        facing = (nx * x + ny * y) + nz * z
        cons = np.isfinite(o).all(axis=1) & ((facing <= 0) if mutant == "facing_le" else (facing < 0))
        if mutant == "round_half_even":
            ui, vi = np.rint(x * fx / z + ppx), np.rint(y * fy / z + ppy)
        elif mutant == "round_truncate":
            ui, vi = np.trunc((x * fx / z + ppx) + 0.5) + 0.0, np.trunc((y * fy / z + ppy) + 0.5) + 0.0   # + 0.0: no -0.0
        else:
            ui = np.floor((x * fx / z + ppx) + 0.5)
            vi = np.floor((y * fy / z + ppy) + 0.5)
        front = np.ones(len(o), dtype=bool) if mutant == "no_z_positive" else o[:, 2] > 0
        inr = cons & front & (ui >= 0) & (ui < depth.shape[1]) & (vi >= 0) & (vi < depth.shape[0])
        d = np.zeros(len(o), dtype=F32)
        d[inr] = depth[vi[inr].astype(np.int64), ui[inr].astype(np.int64)]
        miss = np.abs((d - o[:, 2]).astype(F32))
        valid = np.isfinite(d) if mutant == "no_d_positive" else np.isfinite(d) & (d > 0)
        pair = inr & valid & ((miss < F32(gate)) if mutant == "gate_strict" else (miss <= F32(gate)))
        dd = d.astype(F64)
        q = [(ui - ppx) * dd / fx, (vi - ppy) * dd / fy, dd]
        a = [x - ck[0], y - ck[1], z - ck[2]]
        r = (nx * (q[0] - x) + ny * (q[1] - y)) + nz * (q[2] - z)
        J = [a[1] * nz - a[2] * ny, a[2] * nx - a[0] * nz, a[0] * ny - a[1] * nx, nx, ny, nz]
        J = [np.where(pair, v, 0.0) for v in J]
        r = np.where(pair, r, 0.0)
        cols = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r]
    return chunk_sums(np.stack(cols, axis=1), mutant), int(cons.sum()), int(pair.sum()), ck


def evaluate_loop(rows, T, c0, depth, intr, gate):
    """the 28 sums of evaluate by a plain loop over the rows, one scalar at a time, and chunk_sums_loop: (the sums, the
    (n, 28) products); a second statement of the specification for the tests"""
    fx, fy, ppx, ppy = (float(v) for v in intr)
    T = np.asarray(T, dtype=F64).reshape(4, 4)
    ck = [float(((T[r, 0] * c0[0] + T[r, 1] * c0[1]) + T[r, 2] * c0[2]) + T[r, 3]) for r in range(3)]
    o = transform_rows(rows, T)
    prods = np.zeros((len(rows), ENTRIES))
    with np.errstate(all="ignore"):
        for j in range(len(rows)):
            if not np.isfinite(o[j]).all():
                continue
            x, y, z, nx, ny, nz = (F64(v) for v in o[j])
            if not (nx * x + ny * y) + nz * z < 0 or not z > 0:
                continue
            ui, vi = np.floor((x * fx / z + ppx) + 0.5), np.floor((y * fy / z + ppy) + 0.5)
            if not (0 <= ui < depth.shape[1] and 0 <= vi < depth.shape[0]):
                continue
            d = depth[int(vi), int(ui)]
            if not (np.isfinite(d) and d > 0 and abs(F32(d - o[j, 2])) <= F32(gate)):
                continue
            d = F64(d)
            q = ((ui - ppx) * d / fx, (vi - ppy) * d / fy, d)
            a = (x - ck[0], y - ck[1], z - ck[2])
            r = (nx * (q[0] - x) + ny * (q[1] - y)) + nz * (q[2] - z)
            J = (a[1] * nz - a[2] * ny, a[2] * nx - a[0] * nz, a[0] * ny - a[1] * nx, nx, ny, nz)
            prods[j] = [J[i] * J[k] for i in range(6) for k in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r]
    return chunk_sums_loop(prods), prods


def solve6(tot, mutant=None):
    """icp_solve6_wave: x (6 floats) or None"""
    M = [[0.0] * 7 for _ in range(6)]
    e = 0
    for i in range(6):
        for j in range(i, 6):
            M[i][j] = M[j][i] = float(tot[e])
            e += 1
    for i in range(6):
        M[i][6] = float(tot[21 + i])
    trace = 0.0
    for i in range(6):
        trace = trace + M[i][i]
    if not trace > 0.0:
        return None
    lam = 1e-10 * trace
    for i in range(6):
        M[i][i] = M[i][i] + lam
    for c in range(6):
        piv, pv = c, abs(M[c][c])
        for r in range(c + 1, 6):
            if abs(M[r][c]) > pv or (mutant == "pivot_last" and abs(M[r][c]) == pv):
                piv, pv = r, abs(M[r][c])
        if pv < 1e-300:
            return None
        M[c], M[piv] = M[piv], M[c]
        for r in range(c + 1, 6):
            f = M[r][c] / M[c][c]
            for k in range(c, 7):
                M[r][k] = M[r][k] - f * M[c][k]
    with np.errstate(all="ignore"):
        for c in range(5, -1, -1):
            s = F64(M[c][6])
            for k in range(c + 1, 6):
                s = s - F64(M[c][k]) * F64(M[k][6])
            M[c][6] = float(s / F64(M[c][c]))
    return [M[i][6] for i in range(6)]


def _matmul(A, B, n):
    out = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            s = 0.0
            for k in range(n):
                s = s + A[i][k] * B[k][j]
            out[i][j] = s
    return out


def step_matrix(x, ck):
    """M = [R | (c_k + t) - R c_k], R = Rz(x2) Ry(x1) Rx(x0) by icp_transform_from_euler's arithmetic"""
    sn = oracle_lib.math_eval("sin", np.array(x[:3], dtype=F64))
    cs = oracle_lib.math_eval("cos", np.array(x[:3], dtype=F64))
    cx, cy, cz = (float(v) for v in cs)
    sx, sy, sz = (float(v) for v in sn)
    Rx = [[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]]
    Ry = [[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]
    Rz = [[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]
    R = _matmul(Rz, _matmul(Ry, Rx, 3), 3)
    c = [float(v) for v in ck]
    M = [[R[i][0], R[i][1], R[i][2], (c[i] + x[3 + i]) - ((R[i][0] * c[0] + R[i][1] * c[1]) + R[i][2] * c[2])] for i in range(3)]
    return M + [[0.0, 0.0, 0.0, 1.0]]


def refine(model, T0, depth, intr, p=None, mutant=None, trace=None):
    """(T (4, 4) float64, info dict) of one pose; model (n, 6) float32, depth (rows, cols) float32.  mutant: None, or the
    one rule of MUTANTS to alter; trace: a list that gets (T, n_considered, n_pairs) of every evaluation"""
    assert mutant is None or mutant in MUTANTS, mutant
    p = params(**(p or {}))
    model = np.ascontiguousarray(model, dtype=F32)
    depth = np.ascontiguousarray(depth, dtype=F32)
    rows = model[::p["model_step"]]
    T = np.array(T0, dtype=F64).reshape(4, 4).copy()
    info = dict(status=MAX_ITERS, iterations=0, n_rows=len(rows), n_considered=0, n_pairs_first=0, n_pairs_last=0,
                rmse_first=F32(0), rmse_last=F32(0))
    if p["max_iters"] == 0:
        return T, info
    c0 = centre(model, p["model_step"], mutant)
    lim = {k: float(F32(p[k])) * float(F32(p[k])) for k in ("max_step_rot", "max_step_trans", "eps_rot", "eps_trans")}
    for k in range(p["max_iters"]):
        tot, n_cons, n_pairs, ck = evaluate(rows, T, c0, depth, intr, p["depth_gate"], mutant)
        if trace is not None:
            trace.append((T.copy(), n_cons, n_pairs))
        rmse = F32(np.sqrt(tot[27] / F64(n_pairs))) if n_pairs else F32(0)
        info.update(n_considered=n_cons, n_pairs_last=n_pairs, rmse_last=rmse)
        if k == 0:
            info.update(n_pairs_first=n_pairs, rmse_first=rmse)
        few = n_pairs <= p["min_pairs"] if mutant == "min_pairs_le" else n_pairs < p["min_pairs"]
        share = float(F32(p["min_pair_share"])) * float(n_cons)
        if few or (float(n_pairs) <= share if mutant == "share_le" else float(n_pairs) < share):
            info["status"] = LOST
            return T, info
        x = solve6(tot, mutant)
        if x is None or not all(np.isfinite(x)):
            info["status"] = STEP
            return T, info
        ww = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
        tt = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]
        if ww > lim["max_step_rot"] or tt > lim["max_step_trans"]:
            info["status"] = STEP
            return T, info
        T = np.array(_matmul(step_matrix(x, ck), T.tolist(), 4), dtype=F64)
        info["iterations"] = k + 1
        if ww <= lim["eps_rot"] and tt <= lim["eps_trans"]:
            info["status"] = CONVERGED
            return T, info
    return T, info


# ---- the synthetic case of the issue: an ellipsoid in front of a background ------------------------------------------
def ellipsoid(n=3001, axes=(0.030, 0.045, 0.070), seed=7):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    ax = np.asarray(axes, dtype=F64)
    nrm = u / ax
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.concatenate([u * ax, nrm], axis=1).astype(F32)


def rot_vec(v):
    """the rotation matrix of the rotation vector v (Rodrigues)"""
    t = float(np.linalg.norm(v))
    if t == 0:
        return np.eye(3)
    a = np.asarray(v, dtype=F64) / t
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def offset_pose(T, centre_cam, trans, rot):
    """T followed by the rotation vector `rot` about the camera-frame point `centre_cam`, then the translation `trans`"""
    M = np.eye(4)
    M[:3, :3] = rot_vec(rot)
    M[:3, 3] = centre_cam - M[:3, :3] @ centre_cam + np.asarray(trans, dtype=F64)
    return M @ T


def random_offset(rng, mm, deg):
    """a translation of length mm and a rotation vector of angle deg, both in random directions"""
    t = rng.normal(size=3)
    r = rng.normal(size=3)
    return t / np.linalg.norm(t) * mm * 1e-3, r / np.linalg.norm(r) * np.radians(deg)


def mean_row_error(model, Ta, Tb):
    p = model[:, :3].astype(F64)
    a = p @ np.asarray(Ta)[:3, :3].T + np.asarray(Ta)[:3, 3]
    b = p @ np.asarray(Tb)[:3, :3].T + np.asarray(Tb)[:3, 3]
    return float(np.linalg.norm(a - b, axis=1).mean())
