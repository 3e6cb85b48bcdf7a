"""tests/depth_motion_oracle.py, the numpy restatement of ppf_depth_motion, held to plain per-pixel loops, to known answers and
to the accuracy the proposal measured: the device tests (tests/test_gpu_depth_motion.py) hold the kernels to it byte for byte."""
import numpy as np
import pytest

import depth_motion_cases as Cs
import depth_motion_oracle as O

F32, F64 = np.float32, np.float64
INTR = Cs.intrinsics()

# The worst of the 8 draws of 30 mm / 3 degrees as this oracle measures it (fixed tree, the scene of depth_motion_cases): 0.4843 mm
# and 0.04647 degrees.  The asserted bound is twice that, margin for a tree against plain sums, and has to stay under a quarter
# of the pixel footprint z / fx at 0.7 m: 0.7 / 150 / 4 = 1.17 mm.
MEASURED_WORST_MM, MEASURED_WORST_DEG = 0.4843, 0.04647
BOUND_MM, BOUND_DEG = 2 * MEASURED_WORST_MM, 2 * MEASURED_WORST_DEG
QUARTER_FOOTPRINT_MM = 0.7 / 150.0 / 4.0 * 1e3


def same_rows(a, b):
    return all(np.asarray(ra[f]).tobytes() == np.asarray(rb[f]).tobytes() for ra, rb in zip(a, b) for f in O.ROW_FIELDS)


# ---- the pieces against a second statement -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 60, 64, 65, 135 * 64 - 3, 64 * 64 + 1])
def test_tree_sums_equal_the_lane_loops(n):
    rng = np.random.default_rng(n)
    vals = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-6, 6, size=(n, 3))
    vals[rng.random((n, 3)) < 0.3] = 0.0
    assert O.tree_sums(vals).tobytes() == O.tree_sums_loop(vals).tobytes()


def test_a_single_value_is_its_own_sum_sign_included():
    assert np.signbit(O.tree_sums(np.full((64, 1), -0.0))[0])       # 64 lanes of -0.0: the tree keeps the sign
    assert not np.signbit(O.tree_sums(np.full((63, 1), -0.0))[0])   # lane 63 holds +0.0


def test_down_equals_the_pixel_loop():
    rng = np.random.default_rng(5)
    z = (0.5 + rng.random((9, 11)) * 0.05).astype(F32)
    z[rng.random(z.shape) < 0.3] = 0
    z[2:4, 2:4] = [[0.5, 0.7], [0.52, 0.9]]
    got = O.down(z, 0.03)
    assert got.shape == (4, 5)
    for v in range(4):
        for u in range(5):
            s = [z[2 * v, 2 * u], z[2 * v, 2 * u + 1], z[2 * v + 1, 2 * u], z[2 * v + 1, 2 * u + 1]]
            kept = [x for x in s if x > 0]
            want = F32(0)
            if kept:
                m, tot, cnt = min(kept), 0.0, 0
                for x in kept:
                    if float(x) - float(m) <= float(F32(0.03)):
                        tot, cnt = tot + float(x), cnt + 1
                want = F32(tot / cnt)
            assert got[v, u].tobytes() == want.tobytes(), (v, u)
    assert got[1, 1] == F32((0.5 + float(F32(0.52))) / 2)   # 0.7 and 0.9 lie beyond the gate of the nearest sample


def test_maps_equal_the_pixel_loop():
    prev, _, _ = Cs.pair(0, 30, 3, rows=24, cols=40)
    intr = Cs.intrinsics(24, 40)
    fx, fy, ppx, ppy = intr
    z = O.level0(prev)
    V, n, has = O.maps(z, intr, float(F32(0.01)))
    assert has.sum() > 100 and not has[0].any() and not has[:, -1].any()

    def vert(u, v):
        Z = float(z[v, u])
        return np.array([(float(u) - ppx) * Z / fx, (float(v) - ppy) * Z / fy, Z])

    for v in range(24):
        for u in range(40):
            want, wn = False, np.zeros(3, F32)
            if 0 < u < 39 and 0 < v < 23 and z[v, u] > 0:
                nb = [(u - 1, v), (u + 1, v), (u, v - 1), (u, v + 1)]
                if all(z[b, a] > 0 and abs(float(z[b, a]) - float(z[v, u])) <= float(F32(0.01)) for a, b in nb):
                    dx, dy = vert(u + 1, v) - vert(u - 1, v), vert(u, v + 1) - vert(u, v - 1)
                    c = [dy[1] * dx[2] - dy[2] * dx[1], dy[2] * dx[0] - dy[0] * dx[2], dy[0] * dx[1] - dy[1] * dx[0]]
                    ln = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
                    if ln > 0:
                        nf = np.array([F32(c[k] / ln) for k in range(3)], F32)
                        P = vert(u, v)
                        if (float(nf[0]) * P[0] + float(nf[1]) * P[1]) + float(nf[2]) * P[2] < 0:
                            want, wn = True, nf
            assert has[v, u] == want and n[v, u].tobytes() == wn.tobytes(), (u, v)


def test_level_intrinsics():
    assert O.level_intr((150.0, 140.0, 79.5, 59.5), 2) == (37.5, 35.0, ((79.5 - 0.5) / 2 - 0.5) / 2, ((59.5 - 0.5) / 2 - 0.5) / 2)


def test_launch_counts():
    p = O.params()
    # 720 x 1280: 14,400 -> 225 (one group stage) -> the tail; 360 x 640: 3,600 -> 57; 180 x 320: 900 -> 15
    assert O.group_stages(14400) == 1 and O.group_stages(64) == 0 and O.group_stages(65) == 1 and O.group_stages(64 * 1024 + 1) == 2
    assert O.n_launches((720, 1280), p) == 1 + 2 + 3 + (10 + 5 + 4) * 3
    assert O.n_launches((24, 40), p) == 1 + 2 + 3 + 10 * 2 + 5 * 2 + 4 * 2   # 15, 4 and 1 chunks: no group stage
    assert O.n_launches((24, 40), O.params(iters=(3, 0, 2, 9))) == 6 + 3 * 2 + 1 + 2 * 2


# ---- known answers -----------------------------------------------------------------------------------------------------
def test_identical_images_give_the_identity_byte_for_byte():
    prev, _, _ = Cs.pair(0, 30, 3)
    T, rows, st = O.motion(prev, prev, INTR)
    assert T.tobytes() == np.eye(4).tobytes()
    for l in range(3):
        assert rows[l]["status"] == O.CONVERGED and rows[l]["iterations"] == 1, rows[l]
        assert rows[l]["rmse_first"] == 0 and rows[l]["rmse_last"] == 0
        assert rows[l]["n_pairs_first"] == rows[l]["n_pairs_last"] == rows[l]["n_source"] > 0
        assert (rows[l]["rows"], rows[l]["cols"]) == (120 >> l, 160 >> l)
    assert rows[3] == O.empty_row()
    assert st["status"] == O.CONVERGED and st["n_evaluations"] == 3 and st["n_enqueued"] == 19


def test_an_empty_image_skips_every_level():
    init = Cs.true_motion(3, 10, 1)
    zero = np.zeros((120, 160), F32)
    T, rows, st = O.motion(zero, zero, INTR, init=init)
    assert T.tobytes() == init.tobytes()
    assert [r["status"] for r in rows] == [O.SKIPPED] * 3 + [O.NONE]
    assert all(r["n_source"] == 0 and r["iterations"] == 0 for r in rows)
    assert st["status"] == O.SKIPPED and st["n_evaluations"] == 0


def test_a_start_far_off_is_lost_with_the_start_returned():
    prev, _, _ = Cs.pair(0, 30, 3)
    init = Cs.true_motion(11, 100, 10)
    T, rows, st = O.motion(prev, prev, INTR, init=init)
    assert st["status"] == O.LOST and T.tobytes() == init.tobytes()
    assert rows[2]["status"] == O.LOST and rows[2]["iterations"] == 0 and rows[2]["n_pairs_first"] == rows[2]["n_pairs_last"]
    assert rows[1] == O.empty_row() and rows[0] == O.empty_row()
    assert st["n_evaluations"] == 1


def test_a_step_over_the_limit_ends_the_call():
    """30 mm in one frame against max_step_trans of 1 mm: the first solve asks for more than the limit"""
    prev, cur, _ = Cs.pair(0, 30, 3)
    T, rows, st = O.motion(prev, cur, INTR, dict(max_step_trans=0.001))
    assert st["status"] == O.STEP and T.tobytes() == np.eye(4).tobytes()
    assert rows[2]["status"] == O.STEP and rows[2]["iterations"] == 0 and rows[2]["n_pairs_first"] >= 16
    assert rows[1] == O.empty_row() and st["n_evaluations"] == 1


def test_iters_zero_skips_the_level():
    prev, cur, _ = Cs.pair(0, 30, 3)
    T, rows, st = O.motion(prev, cur, INTR, dict(iters=(10, 0, 4, 4)))
    assert rows[1]["status"] == O.SKIPPED and rows[1]["n_source"] > 0 and rows[1]["n_pairs_first"] == 0
    assert rows[2]["status"] in (O.CONVERGED, O.MAX_ITERS) and rows[0]["status"] in (O.CONVERGED, O.MAX_ITERS)
    assert st["n_enqueued"] == 14


def test_one_level_equals_the_level_0_part_of_three():
    prev, cur, _ = Cs.pair(2, 30, 3)
    trace = []
    T3, rows3, _ = O.motion(prev, cur, INTR, trace=trace)
    start = next(T for l, k, T, _ in trace if l == 0 and k == 0)
    T1, rows1, st1 = O.motion(prev, cur, INTR, dict(levels=1), init=start)
    assert T1.tobytes() == T3.tobytes() and same_rows(rows1[:1], rows3[:1])
    assert rows1[1] == O.empty_row() and st1["n_evaluations"] == sum(1 for l, _, _, _ in trace if l == 0)


def test_max_iters_is_reached():
    prev, cur, _ = Cs.pair(0, 30, 3)
    _, rows, _ = O.motion(prev, cur, INTR, dict(iters=(1, 1, 1, 1)))
    assert [r["status"] for r in rows[:3]] == [O.MAX_ITERS] * 3 and [r["iterations"] for r in rows[:3]] == [1, 1, 1]


# ---- accuracy ----------------------------------------------------------------------------------------------------------
def test_the_bound_stays_under_a_quarter_of_the_pixel_footprint():
    assert BOUND_MM < QUARTER_FOOTPRINT_MM


@pytest.mark.parametrize("seed", Cs.ACCURACY_SEEDS)
def test_accuracy_at_30_mm_and_3_degrees(seed):
    """the analytic scene at 120 x 160, fx = fy = 150, three levels, noise 0.002 z^2, one pixel in twenty dropped"""
    prev, cur, T_true = Cs.pair(seed, 30, 3)
    T, rows, st = O.motion(prev, cur, INTR)
    mm, deg = O.pose_error(T, T_true)
    print(f"seed {seed}: {O.STATUS[st['status']]} {mm:.4f} mm {deg:.5f} deg, {st['n_evaluations']} evaluations")
    assert st["status"] in (O.CONVERGED, O.MAX_ITERS)
    assert all(r["status"] in (O.CONVERGED, O.MAX_ITERS) for r in rows[:3])
    assert mm <= BOUND_MM and deg <= BOUND_DEG


def test_accuracy_without_noise_at_20_mm_and_2_degrees():
    """exact images: what is left is the discretisation of the projective association, far below the noisy figure"""
    worst = 0.0
    for seed in Cs.ACCURACY_SEEDS:
        prev, cur, T_true = Cs.pair(seed, 20, 2, noise=0.0, drop=0.0)
        T, _, st = O.motion(prev, cur, INTR)
        assert st["status"] in (O.CONVERGED, O.MAX_ITERS)
        worst = max(worst, O.pose_error(T, T_true)[0])
    print(f"worst without noise: {worst:.4f} mm")
    assert worst <= MEASURED_WORST_MM
