"""The numpy oracle of ppf_depth_history (tests/depth_history_oracle.py) held to the specification of DESIGN.md §26: against
a per-pixel restatement in Python doubles on seeded image sequences with every kind of invalid value, for every window over
2K + 2 pushes, every min_support, the four kinds of max_age, both modes, the z cuts and 16-bit frames; at the closure of the
gate, on the lower median, on a mean whose bytes depend on the order of the sum, on window 1, on a step change; and on the
synthetic stream the stage was proposed with, whose noise and hole figures it has to reach."""
import math

import numpy as np
import pytest

import depth_history_oracle as H
from depth_normals_oracle import metric_depth

BAD = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -0.5, -1e-30], np.float32)
# four float32 whose fp64 sum rounds differently oldest first and newest first, by age (newest first); they span 2^53
ORDER_BITS = np.array([1417579868, 978599742, 969722779, 1419469303], np.uint32)


def sequence(rng, shape, n_frames, dtype=np.float32):
    """frames of one surface with noise around the default range, pixels that are mostly holes, pixels that never are, holes of
    every invalid kind, and a patch whose depth jumps in mid-sequence"""
    rows, cols = shape
    v, u = np.mgrid[0:rows, 0:cols]
    base = 1.0 + 0.05 * np.sin(u / 7.0) + 0.04 * np.cos(v / 5.0)
    p_hole = rng.choice([0.0, 0.25, 0.6, 0.93], size=shape)
    frames = []
    for t in range(n_frames):
        z = base + 0.006 * rng.normal(size=shape)
        if t >= n_frames // 2:
            z[: (rows + 1) // 2, : (cols + 1) // 2] += 0.2
        drop = rng.random(shape) < p_hole
        if dtype == np.uint16:
            img = np.round(z * 1000.0).astype(np.uint16)
            img[drop] = 0
        else:
            img = z.astype(np.float32)
            img[drop] = BAD[rng.integers(0, len(BAD), size=int(drop.sum()))]
        frames.append(img)
    return frames


def loops_push(frames, *, depth_scale=0.001, z_min=0.0, z_max=0.0, window=8, range_abs=0.01, range_quad=0.0, min_support=1, max_age=7,
               mean=False):
    """the specification for the newest of `frames` (oldest first), pixel by pixel in Python doubles"""
    zs = [metric_depth(f, depth_scale) for f in frames[-window:]][::-1]          # by age
    n_hist = len(zs)
    rows, cols = zs[0].shape
    zmin, zmax = np.float32(z_min), np.float32(z_max)
    ra, rq = float(np.float32(range_abs)), float(np.float32(range_quad))
    out, state = np.zeros((rows, cols), np.float32), np.zeros((rows, cols), np.uint8)
    for v in range(rows):
        for u in range(cols):
            s = []
            for a in range(n_hist):
                z = zs[a][v, u]
                kept = math.isfinite(z) and z > 0 and z >= zmin and (zmax == 0 or z <= zmax)
                s.append(z if kept else None)
            astar = next((a for a in range(min(max_age, n_hist - 1) + 1) if s[a] is not None), None)
            if astar is None:
                continue
            Za = float(s[astar])
            R = ra + rq * (Za * Za)
            C = [a for a in range(n_hist) if s[a] is not None and abs(float(s[a]) - Za) <= R]
            n = len(C)
            if n < min_support:
                state[v, u] = 3
                continue
            if mean:
                total = 0.0
                for a in range(n_hist - 1, -1, -1):
                    if a in C:
                        total = total + float(s[a])
                out[v, u] = np.float32(total / float(n))
            else:
                out[v, u] = sorted(s[a] for a in C)[(n - 1) // 2]
            state[v, u] = 1 if astar == 0 else 2
            if astar == 0 and n == 1 and any(x is not None for x in s[1:]):
                state[v, u] |= 16
    return out, state


def run_both(frames, **kw):
    """every push of the sequence: the oracle equals the loops, and the counts are the state image's"""
    h = H.History(**kw)
    seen = set()
    for t in range(len(frames)):
        out, state, counts = h.push(frames[t])
        want_out, want_state = loops_push(frames[:t + 1], **kw)
        assert out.tobytes() == want_out.tobytes() and state.tobytes() == want_state.tobytes(), (kw, t)
        assert counts["n_measured"] + counts["n_filled"] + counts["n_unsupported"] + counts["n_empty"] == state.size
        assert counts["frame"] == t and out.dtype == np.float32 and state.dtype == np.uint8
        assert np.array_equal(out != 0, (state & 15 == 1) | (state & 15 == 2))
        seen |= set(np.unique(state).tolist())
    return seen


@pytest.mark.parametrize("window", range(1, 17))
def test_vectorised_form_equals_the_pixel_loops_for_every_window(window):
    rng = np.random.default_rng(200 + window)
    frames = sequence(rng, (5, 7), 2 * window + 2)
    seen = set()
    for min_support in range(1, window + 1):
        max_age = (0, 1, window - 1, 15)[min_support % 4]
        seen |= run_both(frames, window=window, min_support=min_support, max_age=max_age, mean=bool(min_support % 2))
    if window >= 3:
        assert seen >= {0, 1, 2, 3, 17}, seen


@pytest.mark.parametrize("mean", [False, True])
def test_larger_images_quad_term_cuts_and_u16(mean):
    rng = np.random.default_rng(230)
    frames = sequence(rng, (24, 40), 11)
    assert run_both(frames, window=8, mean=mean) >= {0, 1, 2, 17}
    small = sequence(rng, (6, 9), 10)
    run_both(small, window=4, range_abs=0.002, range_quad=0.01, mean=mean, max_age=15)
    run_both(small, window=5, z_min=1.0, z_max=1.06, mean=mean, min_support=2)
    u16 = sequence(rng, (6, 9), 10, dtype=np.uint16)
    run_both(u16, window=3, depth_scale=0.001, mean=mean)
    run_both(u16, window=6, depth_scale=0.000125, range_abs=0.002, z_min=0.12, z_max=0.135, mean=mean)


def one_pixel(samples_oldest_first, **kw):
    h = H.History(**kw)
    for s in samples_oldest_first:
        res = h.push(np.array([[s]], np.float32))
    return res[0][0, 0], int(res[1][0, 0]), res[2]


def test_gate_closure():
    """fabs(s - Za) == R is inside, one ulp further is outside: 1.0, 1.0078125 and range_abs 0.0078125 are exact in float32"""
    far = np.float32(1.0078125)
    out, state, _ = one_pixel([far, np.float32(1.0)], range_abs=0.0078125, mean=True, window=2)
    assert out == np.float32((1.0 + 1.0078125) / 2) and state == 1
    out, state, _ = one_pixel([np.nextafter(far, np.float32(2)), np.float32(1.0)], range_abs=0.0078125, mean=True, window=2)
    assert out == np.float32(1.0) and state == 17
    # the quad term takes part: R = 0.00390625 + 0.00390625 * 1.0 * 1.0
    out, state, _ = one_pixel([far, np.float32(1.0)], range_abs=0.00390625, range_quad=0.00390625, mean=True, window=2)
    assert out == np.float32((1.0 + 1.0078125) / 2) and state == 1


def test_lower_median_of_an_even_count():
    s = [np.float32(x) for x in (1.003, 1.0, 1.002, 1.001)]
    out, state, _ = one_pixel(s, window=4)
    assert out.tobytes() == np.float32(1.001).tobytes() and state == 1
    out, _, _ = one_pixel(s[:3], window=4)                     # odd: the middle one
    assert out.tobytes() == np.float32(1.002).tobytes()
    out, _, _ = one_pixel(s[:2], window=4)
    assert out.tobytes() == np.float32(1.0).tobytes()


def order_frames():
    return [np.array([[s]], np.float32) for s in ORDER_BITS.view(np.float32)[::-1]]       # oldest first


def test_the_mean_is_summed_oldest_first():
    by_age = ORDER_BITS.view(np.float32)
    assert by_age.max() / by_age.min() > 2.0 ** 29

    def mean_of(vals):
        total = 0.0
        for x in vals:
            total = total + float(x)
        return np.float32(total / float(len(vals)))
    oldest_first, newest_first = mean_of(by_age[::-1]), mean_of(by_age)
    assert oldest_first.tobytes() != newest_first.tobytes()         # the case does depend on the order
    h = H.History(window=4, range_abs=3e38, mean=True)
    for f in order_frames():
        out, state, counts = h.push(f)
    assert out[0, 0].tobytes() == oldest_first.tobytes() and state[0, 0] == 1


def test_window_one_returns_the_kept_input():
    rng = np.random.default_rng(240)
    h = {m: H.History(window=1, max_age=15, mean=m) for m in (False, True)}
    for f in sequence(rng, (9, 13), 4):
        for m in (False, True):
            out, state, counts = h[m].push(f)
            with np.errstate(invalid="ignore"):
                kept = np.isfinite(f) & (f > 0)
            assert out.tobytes() == np.where(kept, f, np.float32(0)).tobytes()
            assert np.array_equal(state, kept.astype(np.uint8)) and counts["n_changed"] == 0 == counts["n_filled"]


def test_a_step_change_is_followed_in_its_frame():
    shape, t0 = (6, 8), 5
    before = np.full(shape, np.float32(1.0))
    after = before.copy()
    after[2:4, 3:6] = np.float32(0.8)
    for mean in (False, True):
        h = H.History(window=8, mean=mean)
        for t in range(t0 + 3):
            out, state, counts = h.push(after if t >= t0 else before)
            if t == t0:
                assert out.tobytes() == after.tobytes()
                assert np.array_equal(state & 16 != 0, after != before) and counts["n_changed"] == 6
            else:
                assert not (state & 16).any() and out.tobytes() == (after if t > t0 else before).tobytes()
            assert np.array_equal(state & 15, np.ones(shape, np.uint8))


def evidence_stream():
    """the stream of the proposal: a 360 x 640 ramp, 40 empty columns, noise 0.002 D^2, one pixel in ten dropped per frame"""
    rng = np.random.default_rng(7)
    D = np.broadcast_to(0.5 + np.arange(640) / 639.0, (360, 640)).copy()
    D[:, :40] = 0.0
    frames = []
    for _ in range(17):
        z = (D + 0.002 * D * D * rng.standard_normal(D.shape)).astype(np.float32)
        z[rng.random(D.shape) < 0.1] = 0
        frames.append(z)
    return D, frames


EVIDENCE = {}     # mode -> [(push, ratio, holes single, holes fused, n_filled)]: DESIGN.md §26 quotes these


@pytest.mark.parametrize("mean,bound", [(True, 0.45), (False, 0.55)])
def test_evidence_noise_and_holes_on_the_proposed_stream(mean, bound):
    D, frames = evidence_stream()
    valid = D > 0
    h = H.History(window=8, range_abs=0.002, range_quad=0.008, max_age=7, min_support=1, mean=mean)
    rows = []
    for t, f in enumerate(frames):
        out, state, counts = h.push(f)
        if t + 1 not in (8, 17):
            continue
        single = valid & (f > 0)
        holes = int((valid & (f == 0)).sum())
        rms_single = math.sqrt(float(np.mean((f[single].astype(np.float64) - D[single]) ** 2)))
        rms_fused = math.sqrt(float(np.mean((out[valid].astype(np.float64) - D[valid]) ** 2)))
        left = int((valid & (out == 0)).sum())
        rows.append((t + 1, round(rms_fused / rms_single, 3), holes, left, counts["n_filled"]))
        print(f"mean={mean} push {t + 1}: ratio {rms_fused / rms_single:.4f}, single-frame holes {holes}, left {left}, filled {counts['n_filled']}")
        assert rms_fused / rms_single <= bound
        assert left == 0 and counts["n_filled"] == holes and holes > 15000
        assert counts["n_empty"] == int((~valid).sum()) and counts["n_unsupported"] == 0
    EVIDENCE[mean] = rows
