"""A second source for the Hough accumulators.  TEST INFRASTRUCTURE ONLY.

The voting specification restated in numpy, vectorised over the paired points of a reference point:
feature -> 4 ints -> MurmurHash3_x64_128 (seed 42) low word -> `hash % slots` bucket walk without key comparison -> alpha
difference binned over 4 pi -> flat accumulator index; an index of bin `numAngles` counts in the next model row's bin 0, one
past the buffer is dropped.  Nothing here is shared with oracle_lib or the C++ oracle: the elementary functions are numpy's,
the hash is written out again, the table is a sort by bucket instead of chained lists.
"""
from __future__ import annotations

import math

import numpy as np

EPS = 1.192092896e-07  # FLT_EPSILON as a double: pairs closer than this keep the all-zero feature
_C1, _C2 = np.uint64(0x87C37B91114253D5), np.uint64(0x4CF5AD432745937F)


def _rotl(x, r):
    return (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def _fmix(k):
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xFF51AFD7ED558CCD)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xC4CEB9FE1A85EC53)
    return k ^ (k >> np.uint64(33))


def murmur_low32(keys: np.ndarray) -> np.ndarray:
    """MurmurHash3_x64_128 of rows of four int32 (16 bytes, little endian), seed 42: the low 32 bits of h1."""
    with np.errstate(over="ignore"):
        w = keys.astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
        k1 = w[:, 0] | (w[:, 1] << np.uint64(32))
        k2 = w[:, 2] | (w[:, 3] << np.uint64(32))
        h1 = np.full(k1.shape, 42, dtype=np.uint64)
        h2 = h1.copy()
        k1 = _rotl(k1 * _C1, 31) * _C2
        h1 = h1 ^ k1
        h1 = (_rotl(h1, 27) + h2) * np.uint64(5) + np.uint64(0x52DCE729)
        k2 = _rotl(k2 * _C2, 33) * _C1
        h2 = h2 ^ k2
        h2 = (_rotl(h2, 31) + h1) * np.uint64(5) + np.uint64(0x38495AB5)
        h1 = h1 ^ np.uint64(16)
        h2 = h2 ^ np.uint64(16)
        h1 = h1 + h2
        h2 = h2 + h1
        h1, h2 = _fmix(h1), _fmix(h2)
        return ((h1 + h2) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _trunc_i32(x):
    """(int) of a double as x86-64 evaluates it: towards zero, NaN and out of range give INT_MIN."""
    ok = np.isfinite(x) & (x > -2147483649.0) & (x < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), -2147483648.0).astype(np.int64).astype(np.int32)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def pair_keys(p1, n1, p2, n2, angle_step, dist_step):
    """The four quantised features of the pairs (one first point, many second points)."""
    d = p2 - p1
    f3 = np.sqrt(_dot(d, d))
    far = f3 > EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        dn = d * (1.0 / f3)[:, None]
        f0 = np.where(far, np.arccos(_dot(np.broadcast_to(n1, dn.shape), dn)), 0.0)
        f1 = np.where(far, np.arccos(_dot(n2, dn)), 0.0)
        f2 = np.where(far, np.arccos(_dot(np.broadcast_to(n1, n2.shape), n2)), 0.0)
    return np.stack([_trunc_i32(f0 / angle_step), _trunc_i32(f1 / angle_step), _trunc_i32(f2 / angle_step),
                     _trunc_i32(f3 / dist_step)], axis=1)


def frame(p, n):
    """Rotation taking n onto +x (Rodrigues about (0, n.z, -n.y)) and t = -R p."""
    ang = math.acos(n[0])
    ax = np.array([0.0, n[2], -n[1]])
    if n[1] == 0 and n[2] == 0:
        ax = np.array([0.0, 1.0, 0.0])
    else:
        nrm = math.sqrt(float(_dot(ax, ax)))
        if nrm > EPS:
            ax = ax * (1.0 / nrm)
    s, c = math.sin(ang), math.cos(ang)
    K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    R = c * np.eye(3) + s * K + (1.0 - c) * np.outer(ax, ax)
    Rp = np.array([_dot(R[k], p) for k in range(3)])
    return R, -Rp


def alphas(R, t, p2):
    """Angle of the second points about the first point's normal, in the first point's frame; NaN where undefined."""
    qy = t[1] + (R[1, 0] * p2[:, 0] + R[1, 1] * p2[:, 1] + R[1, 2] * p2[:, 2])
    qz = t[2] + (R[2, 0] * p2[:, 0] + R[2, 1] * p2[:, 1] + R[2, 2] * p2[:, 2])
    a = np.arctan2(-qz, qy)
    a = np.where(np.sin(a) * qz < 0.0, -a, a)
    return -a


class Voter:
    """A trained table: every ordered model pair (i, j), j != i, sorted by its bucket `hash % slots`."""

    def __init__(self, model: np.ndarray, relative_sampling_step: float, num_angles: int = 30):
        m32 = np.ascontiguousarray(model, dtype=np.float32)
        self.model = m32.astype(np.float64)
        self.N, self.A = m32.shape[0], int(num_angles)
        self.angle_step = (360.0 / num_angles) * math.pi / 180.0
        ext = m32[:, :3].max(0) - m32[:, :3].min(0)  # float32, like the diameter built from it
        diameter = np.sqrt(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2], dtype=np.float32)
        self.dist_step = float(np.float32(float(diameter) * relative_sampling_step))
        self.slots = max(16, 1 << (self.N * self.N - 1).bit_length())
        rows, buckets, keys, alpha = [], [], [], []
        for i in range(self.N):
            j = np.delete(np.arange(self.N), i)
            p1, n1 = self.model[i, :3], self.model[i, 3:]
            k = pair_keys(p1, n1, self.model[j, :3], self.model[j, 3:], self.angle_step, self.dist_step)
            R, t = frame(p1, n1)
            a = alphas(R, t, self.model[j, :3])
            rows.append(np.full(j.shape, i, dtype=np.int64))
            keys.append(k)
            buckets.append(murmur_low32(k).astype(np.int64) % self.slots)
            alpha.append(np.where(np.isnan(a), 0.0, a).astype(np.float32).astype(np.float64))  # stored as float
        rows, buckets, alpha = np.concatenate(rows), np.concatenate(buckets), np.concatenate(alpha)
        keys = np.concatenate(keys)
        order = np.argsort(buckets, kind="stable")
        self.e_row, self.e_alpha, self.e_key = rows[order], alpha[order], keys[order]
        self.b_ids, self.b_start, self.b_count = np.unique(buckets[order], return_index=True, return_counts=True)

    def accumulator(self, scene: np.ndarray, i: int, paired: np.ndarray | None = None):
        """(accumulator (N, A) uint32, facts) of the scene's reference point i.  facts: votes cast, spills kept in range,
        spills dropped past the buffer, and votes through buckets that hold model pairs of more than one quantised key."""
        sc = np.ascontiguousarray(scene, dtype=np.float32)
        pr = sc if paired is None else np.ascontiguousarray(paired, dtype=np.float32)
        if paired is None:
            keep = np.arange(pr.shape[0]) != i
        else:
            keep = ~(pr[:, :6] == sc[i, :6]).all(axis=1) | np.isnan(pr[:, :6]).any(axis=1)
        p1, n1 = sc[i, :3].astype(np.float64), sc[i, 3:6].astype(np.float64)
        p2, n2 = pr[keep, :3].astype(np.float64), pr[keep, 3:6].astype(np.float64)
        b = murmur_low32(pair_keys(p1, n1, p2, n2, self.angle_step, self.dist_step)).astype(np.int64) % self.slots
        R, t = frame(p1, n1)
        a_s = alphas(R, t, p2)
        ok = ~np.isnan(a_s)
        b, a_s = b[ok], a_s[ok]
        pos = np.searchsorted(self.b_ids, b)
        pos[pos == len(self.b_ids)] = 0
        hit = self.b_ids[pos] == b
        pos, a_s = pos[hit], a_s[hit]
        cnt = self.b_count[pos]
        # every (hit, entry of its bucket)
        ent = np.repeat(self.b_start[pos], cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        a = self.e_alpha[ent] - np.repeat(a_s, cnt)
        bins = _trunc_i32(self.A * (a + 2.0 * math.pi) / (4.0 * math.pi)).astype(np.int64)
        flat = self.e_row[ent] * self.A + bins
        size = self.N * self.A
        inside = (flat >= 0) & (flat < size)
        acc = np.bincount(flat[inside], minlength=size).astype(np.uint32).reshape(self.N, self.A)
        mixed = np.array([len(np.unique(self.e_key[s:s + c], axis=0)) > 1
                          for s, c in zip(self.b_start[np.unique(pos)], self.b_count[np.unique(pos)])], dtype=bool)
        facts = {"votes": int(inside.sum()), "spills_kept": int((inside & (bins == self.A)).sum()),
                 "spills_dropped": int((~inside & (bins == self.A)).sum()),
                 "mixed_buckets": int(mixed.sum())}
        return acc, facts
