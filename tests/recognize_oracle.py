"""numpy restatement of ppf_recognize_frame's specification (include/ppf_hip.h).  TEST INFRASTRUCTURE ONLY.

Every operation is a single fp64 numpy operation in the order the specification writes it (numpy fuses nothing); acos is
the deterministic one of include/ppf_detmath.h, evaluated through oracle_lib.math_eval.  Nothing here is shared with the
product.
"""
from __future__ import annotations

import math

import numpy as np

import oracle_lib as O

INT32_MIN = -(2 ** 31)
EPS = 1.192092896e-07  # FLT_EPSILON: ppf_pair_feature leaves the angles 0 up to this distance


def d2i(x) -> np.ndarray:
    """ppf_d2i: truncation, INT32_MIN for NaN and whatever does not fit"""
    x = np.asarray(x, dtype=np.float64)
    ok = (x > -2147483649.0) & (x < 2147483648.0)
    out = np.full(x.shape, INT32_MIN, dtype=np.int64)
    out[ok] = np.trunc(x[ok]).astype(np.int64)
    return out.astype(np.int32)


def pair_features(rows) -> np.ndarray:
    """(n, n, 4) float64: ppf_pair_feature of every ordered pair (i, j) of the float rows, f zeroed; the diagonal is included
    (the callers leave it out)"""
    r = np.asarray(rows, dtype=np.float32).astype(np.float64)
    p, nr = r[:, 0:3], r[:, 3:6]
    with np.errstate(all="ignore"):
        dx = p[None, :, 0] - p[:, None, 0]
        dy = p[None, :, 1] - p[:, None, 1]
        dz = p[None, :, 2] - p[:, None, 2]
        f3 = np.sqrt((dx * dx + dy * dy) + dz * dz)
        far = ~(f3 <= EPS)
        s = 1.0 / f3
        dx, dy, dz = dx * s, dy * s, dz * s
        n1x, n1y, n1z = nr[:, None, 0], nr[:, None, 1], nr[:, None, 2]
        n2x, n2y, n2z = nr[None, :, 0], nr[None, :, 1], nr[None, :, 2]
        d0 = (n1x * dx + n1y * dy) + n1z * dz
        d1 = (n2x * dx + n2y * dy) + n2z * dz
        d2 = (n1x * n2x + n1y * n2y) + n1z * n2z + np.zeros_like(dx)
    f = np.zeros(dx.shape + (4,), dtype=np.float64)
    f[..., 3] = f3
    for k, d in enumerate((d0, d1, d2)):
        f[..., k][far] = O.math_eval("acos", d[far])
    return f


def quantise(f, angle_step: float, dist_step: float) -> np.ndarray:
    """the key tuples (int32) of features f (..., 4)"""
    with np.errstate(all="ignore"):
        return np.stack([d2i(f[..., 0] / angle_step), d2i(f[..., 1] / angle_step), d2i(f[..., 2] / angle_step),
                         d2i(f[..., 3] / dist_step)], axis=-1)


def off_diagonal(a) -> np.ndarray:
    """(n, n, ...) -> (n (n - 1), ...): the ordered pairs i != j"""
    n = a.shape[0]
    return a[~np.eye(n, dtype=bool)]


def key_set(rows, angle_step: float, dist_step: float) -> np.ndarray:
    """a model's key set: the distinct keys of all ordered pairs of its sampled rows, in lexicographic order"""
    k = off_diagonal(quantise(pair_features(rows), angle_step, dist_step))
    return np.unique(k.reshape(-1, 4), axis=0)


def used_rows(cloud, max_rows: int) -> np.ndarray:
    """the candidates 0, s, 2s, ... with s = ceil(n / max_rows), those with six finite values"""
    c = np.asarray(cloud, dtype=np.float32).reshape(-1, 6)
    n = c.shape[0]
    if n == 0:
        return c
    s = -(-n // max_rows)
    cand = c[::s]
    return cand[np.isfinite(cand).all(axis=1)]


def counts_from_features(f_pairs, keys, angle_step: float, dist_step: float):
    """(n_known, n_keys_hit) of pair features (P, 4) against a key set (K, 4)"""
    pk = quantise(f_pairs, angle_step, dist_step).reshape(-1, 4)
    if pk.shape[0] == 0 or keys.shape[0] == 0:
        return 0, 0
    # A tuple is compared as one integer: per column the value's rank among the values the key set has in that column (a
    # value the set does not have there cannot belong to a key of the set), the four ranks in mixed radix.
    code_set = np.zeros(keys.shape[0], dtype=np.int64)
    code = np.zeros(pk.shape[0], dtype=np.int64)
    possible = np.ones(pk.shape[0], dtype=bool)
    for col in range(4):
        vals = np.unique(keys[:, col])
        code_set = code_set * vals.shape[0] + np.searchsorted(vals, keys[:, col])
        r = np.minimum(np.searchsorted(vals, pk[:, col]), vals.shape[0] - 1)
        possible &= vals[r] == pk[:, col]
        code = code * vals.shape[0] + r
    known = possible & np.isin(code, code_set)
    return int(known.sum()), int(np.unique(code[known]).shape[0])


def scores(n_known: int, n_keys_hit: int, n_pairs: int, n_keys: int):
    """(precision, recall, score) from the integers, as the host computes them"""
    if n_pairs == 0:
        return 0.0, 0.0, 0.0
    precision = float(n_known) / float(n_pairs)
    recall = float(n_keys_hit) / float(n_keys)
    return precision, recall, precision * recall


def rank(score_rows, top: int, min_score: float = 0.0, min_precision: float = 0.0):
    """score_rows: per model (precision, recall, score); the candidates' model indices, best first"""
    keep = [m for m, (p, _, s) in enumerate(score_rows) if s >= min_score and p >= min_precision]
    keep.sort(key=lambda m: (-score_rows[m][2], m))
    return keep[:top]


class Model:
    """what the recogniser knows of a trained model: its sampled rows, its steps and, from them, its key set"""

    def __init__(self, sampled, angle_step: float, dist_step: float):
        self.rows = np.asarray(sampled, dtype=np.float32)
        self.angle_step, self.dist_step = float(angle_step), float(dist_step)
        self.keys = key_set(self.rows, self.angle_step, self.dist_step)
        self.n_keys = int(self.keys.shape[0])
        self.n_a = int(math.floor(math.pi / self.angle_step)) + 2
        self.n_d = int(self.keys[:, 3].max()) + 1

    @classmethod
    def from_detector(cls, det):
        """det: an oracle_lib.OracleDetector or the product's PPF3DDetector (both have sampled_model() and info())"""
        info = det.info()
        return cls(det.sampled_model(), info["angle_step"], info["distance_step"])


def recognize(clouds, models, max_rows: int = 512, top: int = 2, min_score: float = 0.0, min_precision: float = 0.0):
    """Per cloud (an (n, 6) array or None) a dict: n_used, counts (n_models, 2) uint64, scores (n_models, 3) float64 =
    precision, recall, score, and ranked = the candidates' model indices."""
    out = []
    for c in clouds:
        n_rows = 0 if c is None else np.asarray(c).reshape(-1, 6).shape[0]
        u = used_rows(c, max_rows) if n_rows else np.zeros((0, 6), np.float32)
        n_used = u.shape[0]
        n_pairs = n_used * (n_used - 1)
        f = off_diagonal(pair_features(u)) if n_used >= 2 else np.zeros((0, 4))
        cnt = np.zeros((len(models), 2), dtype=np.uint64)
        sc = np.zeros((len(models), 3), dtype=np.float64)
        for m, md in enumerate(models):
            cnt[m] = counts_from_features(f, md.keys, md.angle_step, md.dist_step)
            sc[m] = scores(int(cnt[m, 0]), int(cnt[m, 1]), n_pairs, md.n_keys)
        ranked = rank([tuple(r) for r in sc], top, min_score, min_precision) if n_rows else []
        out.append({"n_used": n_used, "counts": cnt, "scores": sc, "ranked": ranked})
    return out
