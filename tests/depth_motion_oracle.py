"""A numpy restatement of ppf_depth_motion (the comment above it in include/ppf_hip.h): the camera's motion
between two depth images by projective point-to-plane ICP over a small pyramid.  Every step is the fp64 / fp32 arithmetic the
kernels do, in the same order: products are rounded before they are added (numpy never fuses), the 28 sums go through the
fixed tree (lanes of a chunk, chunks of a group, ... until one value is left), and the solve and the pose update are
refine_oracle's scalars.  sin / cos come from the CPU checker's detmath (oracle_lib.math_eval)."""
import numpy as np

import oracle_lib
from refine_oracle import _matmul, solve6

NONE, CONVERGED, MAX_ITERS, LOST, STEP, SKIPPED = 0, 1, 2, 3, 4, 5
STATUS = {NONE: "NONE", CONVERGED: "CONVERGED", MAX_ITERS: "MAX_ITERS", LOST: "LOST", STEP: "STEP", SKIPPED: "SKIPPED"}
CHUNK, ENTRIES, MAX_LEVELS = 64, 28, 4
TAIL_MAX = 1024   # partial rows the last kernel takes (DM_TAIL_MAX): only the launch count depends on it
F32, F64 = np.float32, np.float64
DEFAULTS = dict(levels=3, iters=(10, 5, 4, 4), pyr_gate=0.03, normal_gate=0.01, dist_gate=0.05, normal_cos=0.8, max_step_rot=0.3,
                max_step_trans=0.15, eps_rot=1e-5, eps_trans=1e-5, min_pair_share=0.25, min_pairs=16)
ROW_FIELDS = ["status", "iterations", "rows", "cols", "n_source", "n_pairs_first", "n_pairs_last", "rmse_first", "rmse_last"]


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **kw)
    p["iters"] = tuple(int(v) for v in p["iters"])
    return p


def empty_row():
    return dict(status=NONE, iterations=0, rows=0, cols=0, n_source=0, n_pairs_first=0, n_pairs_last=0, rmse_first=F32(0), rmse_last=F32(0))


def level0(img, depth_scale=0.001, z_min=0.0, z_max=0.0):
    """step 1: the float z of every kept pixel (ppf_cloud_from_depth's z and "kept"), 0 elsewhere"""
    img = np.asarray(img)
    with np.errstate(all="ignore"):
        z = (img.astype(F64) * F64(depth_scale)).astype(F32) if img.dtype == np.uint16 else img.astype(F32)
        keep = np.isfinite(z) & (z > 0) & (z >= F32(z_min))
        if F32(z_max) != 0:
            keep &= z <= F32(z_max)
    return np.where(keep, z, F32(0)).astype(F32)


def down(z, pyr_gate):
    """step 2: level l -> l + 1"""
    r, c = z.shape[0] // 2, z.shape[1] // 2
    z = z[:2 * r, :2 * c]
    s = [z[0::2, 0::2], z[0::2, 1::2], z[1::2, 0::2], z[1::2, 1::2]]   # (2u, 2v), (2u+1, 2v), (2u, 2v+1), (2u+1, 2v+1)
    kept = [v > 0 for v in s]
    m = np.full((r, c), np.inf)
    for v, k in zip(s, kept):
        m = np.where(k & (v.astype(F64) < m), v.astype(F64), m)
    gate = float(F32(pyr_gate))
    total, cnt = np.zeros((r, c), F64), np.zeros((r, c), np.int64)
    with np.errstate(all="ignore"):
        for v, k in zip(s, kept):
            take = k & (v.astype(F64) - m <= gate)
            total = np.where(take, total + v.astype(F64), total)
            cnt += take
        return np.where(cnt > 0, total / np.maximum(cnt, 1).astype(F64), 0.0).astype(F32)


def level_intr(intr, l):
    fx, fy, ppx, ppy = (float(v) for v in intr)
    for _ in range(l):
        fx, fy, ppx, ppy = fx / 2.0, fy / 2.0, (ppx - 0.5) / 2.0, (ppy - 0.5) / 2.0
    return fx, fy, ppx, ppy


def vertices(z, intr):
    fx, fy, ppx, ppy = intr
    Z = z.astype(F64)
    u = np.arange(z.shape[1], dtype=F64)[None, :]
    v = np.arange(z.shape[0], dtype=F64)[:, None]
    return [(u - ppx) * Z / fx, (v - ppy) * Z / fy, Z]


def maps(z, intr, ngate):
    """step 3: (V: three (rows, cols) float64; n: (rows, cols, 3) float32, zero without a normal; has: bool)"""
    rows, cols = z.shape
    V = vertices(z, intr)
    n = np.zeros((rows, cols, 3), F32)
    has = np.zeros((rows, cols), bool)
    if rows < 3 or cols < 3:
        return V, n, has
    Z = z.astype(F64)
    c, l, r, up, dn = (slice(1, -1), slice(1, -1)), (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None)), \
        (slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1))
    ok = z[c] > 0
    for q in (l, r, up, dn):
        ok &= (z[q] > 0) & (np.abs(Z[q] - Z[c]) <= ngate)
    with np.errstate(all="ignore"):
        dx = [V[k][r] - V[k][l] for k in range(3)]
        dy = [V[k][dn] - V[k][up] for k in range(3)]
        cr = [dy[1] * dx[2] - dy[2] * dx[1], dy[2] * dx[0] - dy[0] * dx[2], dy[0] * dx[1] - dy[1] * dx[0]]
        ln = np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
        nf = [(cr[k] / ln).astype(F32) for k in range(3)]
        facing = (nf[0].astype(F64) * V[0][c] + nf[1].astype(F64) * V[1][c]) + nf[2].astype(F64) * V[2][c]
        ok &= (ln > 0) & (facing < 0) & ((nf[0] != 0) | (nf[1] != 0) | (nf[2] != 0))
    has[c] = ok
    for k in range(3):
        n[..., k][c] = np.where(ok, nf[k], F32(0))
    return V, n, has


def tree_sums(vals):
    """step 6: vals (n, m) float64, row j = what lane j % 64 of chunk j // 64 holds; the (m,) sums by the fixed tree"""
    v = np.asarray(vals, dtype=F64)
    first = True
    with np.errstate(all="ignore"):
        while first or len(v) > 1:
            first = False
            n, m = v.shape
            nc = (n + CHUNK - 1) // CHUNK
            w = np.zeros((nc * CHUNK, m), F64)   # the lanes past the last row hold +0.0
            w[:n] = v
            w = w.reshape(nc, CHUNK, m)
            for off in (32, 16, 8, 4, 2, 1):
                w = w[:, :off] + w[:, off:2 * off]
            v = w[:, 0]
    return v[0]


def tree_sums_loop(vals):
    """tree_sums by plain loops over lanes, one scalar at a time: a second statement for the tests"""
    out = []
    for e in range(vals.shape[1]):
        v = [float(x) for x in vals[:, e]]
        first = True
        while first or len(v) > 1:
            first = False
            nxt = []
            for c0 in range(0, len(v), CHUNK):
                lanes = [v[c0 + l] if c0 + l < len(v) else 0.0 for l in range(CHUNK)]
                for off in (32, 16, 8, 4, 2, 1):
                    for l in range(off):
                        lanes[l] = lanes[l] + lanes[l + off]
                nxt.append(lanes[0])
            v = nxt
        out.append(v[0])
    return np.array(out, dtype=F64)


def evaluate(src, dst, T, intr, dist_gate, normal_cos):
    """step 5 and 6: one evaluation; src, dst = maps() of prev and cur at this level: (the 28 sums, n_pairs, the pair mask)"""
    fx, fy, ppx, ppy = intr
    Vs, ns, has = src
    Vt, nt_all, has_t = dst
    rows, cols = has.shape
    T = np.asarray(T, dtype=F64).reshape(4, 4)
    V = [a.reshape(-1) for a in Vs]
    n = [ns[..., k].reshape(-1).astype(F64) for k in range(3)]
    with np.errstate(all="ignore"):
        p = [((T[r, 0] * V[0] + T[r, 1] * V[1]) + T[r, 2] * V[2]) + T[r, 3] for r in range(3)]
        nn = [(T[r, 0] * n[0] + T[r, 1] * n[1]) + T[r, 2] * n[2] for r in range(3)]
        ui = np.floor((p[0] * fx / p[2] + ppx) + 0.5)
        vi = np.floor((p[1] * fy / p[2] + ppy) + 0.5)
        ok = has.reshape(-1) & (p[2] > 0) & (ui >= 0) & (ui < cols) & (vi >= 0) & (vi < rows)
        iu = np.where(ok, ui, 0).astype(np.int64)
        iv = np.where(ok, vi, 0).astype(np.int64)
        ok &= has_t[iv, iu]
        q = [Vt[k][iv, iu] for k in range(3)]
        nt = [nt_all[iv, iu, k].astype(F64) for k in range(3)]
        dq = [q[k] - p[k] for k in range(3)]
        d2 = (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2]
        cs = (nn[0] * nt[0] + nn[1] * nt[1]) + nn[2] * nt[2]
        dg = float(F32(dist_gate))
        pair = ok & (d2 <= dg * dg) & (cs >= float(F32(normal_cos)))
        r = (nt[0] * dq[0] + nt[1] * dq[1]) + nt[2] * dq[2]
        J = [p[1] * nt[2] - p[2] * nt[1], p[2] * nt[0] - p[0] * nt[2], p[0] * nt[1] - p[1] * nt[0], nt[0], nt[1], nt[2]]
        J = [np.where(pair, v, 0.0) for v in J]
        r = np.where(pair, r, 0.0)
        prods = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * r for i in range(6)] + [r * r]
    return tree_sums(np.stack(prods, axis=1)), int(pair.sum()), pair.reshape(rows, cols)


def step_matrix(x):
    """M = [R | x3 x4 x5], R = Rz(x2) Ry(x1) Rx(x0) by icp_transform_from_euler's arithmetic"""
    sn = oracle_lib.math_eval("sin", np.array(x[:3], dtype=F64))
    cs = oracle_lib.math_eval("cos", np.array(x[:3], dtype=F64))
    cx, cy, cz = (float(v) for v in cs)
    sx, sy, sz = (float(v) for v in sn)
    Rx = [[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]]
    Ry = [[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]
    Rz = [[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]
    R = _matmul(Rz, _matmul(Ry, Rx, 3), 3)
    return [[R[i][0], R[i][1], R[i][2], float(x[3 + i])] for i in range(3)] + [[0.0, 0.0, 0.0, 1.0]]


def pyramid(img, intr, p, depth_scale=0.001, z_min=0.0, z_max=0.0):
    """steps 1 to 3: per level (intrinsics, maps of the image)"""
    z = level0(img, depth_scale, z_min, z_max)
    out = []
    for l in range(p["levels"]):
        if l:
            z = down(z, p["pyr_gate"])
        li = level_intr(intr, l)
        out.append((li, maps(z, li, float(F32(p["normal_gate"])) * float(1 << l))))
    return out


def run_levels(pp, pc, T, p, level_range, rows, trace=None):
    """steps 4 to 7 over the given levels (coarse to fine) on the pyramids pp (prev) and pc (cur): (T, the last status, the
    evaluations run, ended); fills rows[l]"""
    lim = {k: float(F32(p[k])) * float(F32(p[k])) for k in ("max_step_rot", "max_step_trans", "eps_rot", "eps_trans")}
    last, n_eval = NONE, 0
    for l in level_range:
        intr, src = pp[l]
        dst = pc[l][1]
        n_source = int(src[2].sum())
        row = rows[l]
        row.update(rows=src[2].shape[0], cols=src[2].shape[1], n_source=n_source)
        if p["iters"][l] == 0 or n_source < p["min_pairs"]:
            row["status"] = last = SKIPPED
            continue
        for k in range(p["iters"][l]):
            tot, n_pairs, _ = evaluate(src, dst, T, intr, p["dist_gate"], p["normal_cos"])
            n_eval += 1
            if trace is not None:
                trace.append((l, k, T.copy(), n_pairs))
            rmse = F32(np.sqrt(tot[27] / F64(n_pairs))) if n_pairs else F32(0)
            row.update(n_pairs_last=n_pairs, rmse_last=rmse)
            if k == 0:
                row.update(n_pairs_first=n_pairs, rmse_first=rmse)
            if n_pairs < p["min_pairs"] or float(n_pairs) < float(F32(p["min_pair_share"])) * float(n_source):
                row["status"] = LOST
                return T, LOST, n_eval, True
            x = solve6(tot)
            if x is None or not all(np.isfinite(x)):
                row["status"] = STEP
                return T, STEP, n_eval, True
            ww = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
            tt = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]
            if ww > lim["max_step_rot"] or tt > lim["max_step_trans"]:
                row["status"] = STEP
                return T, STEP, n_eval, True
            T = np.array(_matmul(step_matrix(x), T.tolist(), 4), dtype=F64)
            row["iterations"] = k + 1
            if ww <= lim["eps_rot"] and tt <= lim["eps_trans"]:
                row["status"] = last = CONVERGED
                break
            if k + 1 == p["iters"][l]:
                row["status"] = last = MAX_ITERS
        # CONVERGED and MAX_ITERS go on to the next finer level
    return T, last, n_eval, False


def motion(prev, cur, intr, p=None, init=None, depth_scale=0.001, z_min=0.0, z_max=0.0, trace=None):
    """(T (4, 4) float64, the four level rows (dicts of ROW_FIELDS), stats dict) of one call"""
    p = params(**(p or {}))
    T = np.eye(4) if init is None else np.array(init, dtype=F64).reshape(4, 4).copy()
    rows = [empty_row() for _ in range(MAX_LEVELS)]
    pp = pyramid(prev, intr, p, depth_scale, z_min, z_max)
    pc = pyramid(cur, intr, p, depth_scale, z_min, z_max)
    T, last, n_eval, _ = run_levels(pp, pc, T, p, range(p["levels"] - 1, -1, -1), rows, trace)
    stats = dict(status=last, n_evaluations=n_eval, n_enqueued=sum(p["iters"][:p["levels"]]),
                 n_launches=n_launches(np.asarray(prev).shape, p), n_host_syncs=1)
    return T, rows, stats


def group_stages(n_chunks):
    """the k_motion_group launches of one evaluation over n_chunks chunks"""
    n, stages = n_chunks, 0
    if n > CHUNK:
        while True:
            n = (n + CHUNK - 1) // CHUNK
            stages += 1
            if n <= TAIL_MAX:
                break
    return stages


def n_launches(shape, p):
    """the kernel launches of a call: level 0, the reductions, the maps, then per evaluation eval + group stages + tail; a level
    with no evaluation gets the one launch that marks it"""
    p = params(**p)
    rows, cols = shape
    total = 1 + (p["levels"] - 1) + p["levels"]
    for l in range(p["levels"]):
        chunks = (rows * cols + CHUNK - 1) // CHUNK
        total += 1 if p["iters"][l] == 0 else p["iters"][l] * (2 + group_stages(chunks))
        rows, cols = rows // 2, cols // 2
    return total


def pose_error(T, T_true):
    """(translation error in mm, rotation error in degrees) of T against T_true"""
    T, T_true = np.asarray(T, F64).reshape(4, 4), np.asarray(T_true, F64).reshape(4, 4)
    dR = T[:3, :3] @ T_true[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]) * 1e3), float(ang)
