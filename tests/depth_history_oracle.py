"""ppf_depth_history restated in numpy, vectorised over the image and looping over the ages in the specified
order: the anchor is the youngest kept sample up to max_age, the consensus is every remembered sample within R of it, the
value its lower median (no arithmetic) or its mean (one fp64 sum, oldest first).  fp64 + - * / evaluated as written, nothing
fused; the parameters are the float32 values the C record holds, widened.  The device is held to this byte for byte."""
import numpy as np

from depth_normals_oracle import keep_mask, metric_depth

DEFAULTS = dict(window=8, range_abs=0.01, range_quad=0.0, min_support=1, max_age=7, mean=False)
MEASURED, FILLED, UNSUPPORTED, CHANGED = 1, 2, 3, 16
COUNTS = ("n_kept", "n_measured", "n_filled", "n_unsupported", "n_empty", "n_changed", "frame")


def _f32(v):
    return np.float64(np.float32(v))


class History:
    """push(depth) -> (out float32, state uint8, dict of COUNTS); reset(); frames newest first, at most `window` of them"""

    def __init__(self, *, depth_scale=0.001, z_min=0.0, z_max=0.0, window=8, range_abs=0.01, range_quad=0.0, min_support=1, max_age=7,
                 mean=False):
        self.depth = dict(depth_scale=depth_scale, z_min=z_min, z_max=z_max)
        self.window, self.min_support, self.max_age, self.mean = int(window), int(min_support), int(max_age), bool(mean)
        self.range_abs, self.range_quad = _f32(range_abs), _f32(range_quad)
        self.reset()

    def reset(self):
        self.frames, self.t = [], 0

    def push(self, depth):
        z = metric_depth(depth, self.depth["depth_scale"])
        keep = keep_mask(z, self.depth["z_min"], self.depth["z_max"])
        self.frames.insert(0, (np.where(keep, z, np.float32(0)).astype(np.float32), keep))
        del self.frames[self.window:]
        out, state = fuse(self.frames, self.range_abs, self.range_quad, self.min_support, self.max_age, self.mean)
        counts = count(state, keep)
        counts["frame"] = self.t
        self.t += 1
        return out, state, counts


def count(state, keep):
    kind = state & 15
    return dict(n_kept=int(keep.sum()), n_measured=int((kind == MEASURED).sum()), n_filled=int((kind == FILLED).sum()),
                n_unsupported=int((kind == UNSUPPORTED).sum()), n_empty=int((kind == 0).sum()), n_changed=int(((state & CHANGED) != 0).sum()))


def fuse(frames, range_abs, range_quad, min_support, max_age, mean):
    """frames: [(z float32 with 0 where not kept, kept mask)] by age, newest first (n_hist of them)"""
    n_hist = len(frames)
    shape = frames[0][0].shape
    astar = np.full(shape, -1, np.int64)
    za = np.zeros(shape, np.float32)
    for a in range(min(max_age, n_hist - 1) + 1):                    # 1. the anchor: the smallest such age
        take = (astar < 0) & frames[a][1]
        astar[take] = a
        za[take] = frames[a][0][take]
    has = astar >= 0
    Za = za.astype(np.float64)
    with np.errstate(all="ignore"):
        R = range_abs + range_quad * (Za * Za)
        inC = [has & k & (np.abs(s.astype(np.float64) - Za) <= R) for s, k in frames]       # 2. the consensus
    n = np.sum(inC, axis=0)
    ok = has & (n >= min_support)                                     # 3. support
    if mean:                                                          # 4. the value
        total = np.zeros(shape, np.float64)
        for a in range(n_hist - 1, -1, -1):
            total = np.where(inC[a], total + frames[a][0].astype(np.float64), total)
        with np.errstate(all="ignore"):
            val = (total / n.astype(np.float64)).astype(np.float32)
    else:
        vals = np.sort(np.stack([np.where(c, s, np.float32(np.inf)) for c, (s, _) in zip(inC, frames)]), axis=0)
        val = np.take_along_axis(vals, (np.maximum(n, 1) - 1)[None] // 2, axis=0)[0]
    out = np.where(ok, val, np.float32(0)).astype(np.float32)
    older = np.zeros(shape, bool)
    for _, k in frames[1:]:
        older |= k
    state = np.zeros(shape, np.uint8)                                 # 5. the state
    state[has & ~ok] = UNSUPPORTED
    state[ok & (astar > 0)] = FILLED
    state[ok & (astar == 0)] = MEASURED
    state[ok & (astar == 0) & (n == 1) & older] |= CHANGED
    return out, state
