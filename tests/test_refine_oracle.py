"""Properties of tests/refine_oracle.py, the numpy statement of DESIGN.md §17, on the CPU: it converges from the starts
ppf_refine_frame is meant for, its guards stop the poses it is not meant for without moving them, it tracks a moved object
past an occluder, and its sums are the ones a plain loop over chunks and lanes gives.

The case: an ellipsoid of 3,001 rows with semi-axes 30 / 45 / 70 mm, 0.6 m from the camera, drawn into a 120 x 160 image
with fx = fy = 300 (a pixel covers z / fx = 2.0 mm there) at 3 mm splats over a background at 0.9 m."""
import numpy as np
import pytest

import refine_oracle as R
import render_oracle as RO

ROWS, COLS = 120, 160
INTR = (300.0, 300.0, 79.5, 59.5)
BACKGROUND = 0.9
FOOTPRINT = 0.6 / 300.0            # metres per pixel at the object
BOUND = FOOTPRINT / 4              # 0.5 mm
STRIP_SHARE = 0.34                 # the occluding strip: 12 of the object's 35 columns (found to hold on the oracle; 18 do not)


def draw(model, T):
    zb = RO.zbuffer(R.transform_rows(model, T), ROWS, COLS, INTR, 0.003)
    depth = zb.view(np.float32).copy()
    depth[zb == RO.EMPTY32] = BACKGROUND
    return depth


@pytest.fixture(scope="module")
def case():
    model = R.ellipsoid(3001, seed=7)
    T = np.eye(4)
    T[:3, :3] = R.rot_vec([0.4, -0.3, 0.2])
    T[:3, 3] = [0.01, -0.005, 0.6]
    centre = T[:3, :3] @ model[:, :3].astype(np.float64).mean(axis=0) + T[:3, 3]
    return dict(model=model, T=T, centre=centre, depth=draw(model, T))


@pytest.mark.parametrize("gate", [0.01, 0.02])
@pytest.mark.parametrize("mm,deg", [(5, 3), (10, 5)])
def test_convergence(case, gate, mm, deg):
    worst, its = 0.0, []
    for seed in range(16):
        t, r = R.random_offset(np.random.default_rng(1000 + seed), mm, deg)
        T0 = R.offset_pose(case["T"], case["centre"], t, r)
        T, info = R.refine(case["model"], T0, case["depth"], INTR, dict(depth_gate=gate))
        err = R.mean_row_error(case["model"], T, case["T"])
        assert info["status"] == R.CONVERGED, (seed, info)
        assert err < BOUND, (seed, err)
        assert info["rmse_last"] < info["rmse_first"]
        worst, its = max(worst, err), its + [info["iterations"]]
    print(f"gate {gate} start ({mm} mm, {deg} deg): worst final {worst * 1e3:.3f} mm, {min(its)}-{max(its)} iterations")


def test_guards(case):
    model, T, depth = case["model"], case["T"], case["depth"]
    far = T.copy()
    far[:3, 3] += [0.04, 0.0, 0.0]
    behind = T.copy()
    behind[2, 3] = -0.6
    nan = T.copy()
    nan[0, 0] = np.nan
    for what, T0, img in (("40 mm", far, depth), ("empty image", T, np.zeros_like(depth)), ("behind", behind, depth), ("nan", nan, depth)):
        got, info = R.refine(model, T0, img, INTR)
        assert info["status"] in (R.LOST, R.STEP), (what, info)
        assert info["iterations"] == 0 and got.tobytes() == np.asarray(T0, dtype=np.float64).tobytes(), what
    # nothing is evaluated with max_iters = 0
    got, info = R.refine(model, far, depth, INTR, dict(max_iters=0))
    assert info["status"] == R.MAX_ITERS and info["iterations"] == 0 and info["n_pairs_first"] == 0 and got.tobytes() == far.tobytes()


@pytest.mark.parametrize("side", ["left", "middle"])
def test_tracking_past_an_occluder(case, side):
    """frame t + 1: the object moved by (4 mm, 2 deg) and a nearer plane covers a strip of a third of its width; the covered
    pixels fail the gate and the pose of frame t still lands on the moved truth"""
    model = case["model"]
    worst = 0.0
    for seed in range(8):
        t, r = R.random_offset(np.random.default_rng(50 + seed), 4, 2)
        T1 = R.offset_pose(case["T"], case["centre"], t, r)
        depth = draw(model, T1)
        cols = np.nonzero((depth < BACKGROUND).any(axis=0))[0]
        width = int(cols[-1] - cols[0] + 1)
        strip = int(np.ceil(STRIP_SHARE * width))
        assert strip * 4 >= width
        s0 = int(cols[0]) if side == "left" else int(cols[0]) + (width - strip) // 2
        free = R.evaluate(model, T1, R.centre(model, 1), depth, INTR, 0.02)
        depth[:, s0:s0 + strip] = 0.45
        covered = R.evaluate(model, T1, R.centre(model, 1), depth, INTR, 0.02)
        assert covered[2] < free[2]   # the covered pixels give no pairs
        T, info = R.refine(model, case["T"], depth, INTR)
        err = R.mean_row_error(model, T, T1)
        assert info["status"] in (R.CONVERGED, R.MAX_ITERS) and err < BOUND, (seed, width, strip, err, info)
        worst = max(worst, err)
    print(f"strip {side}: {strip} of {width} columns, worst final {worst * 1e3:.3f} mm")


@pytest.mark.parametrize("n", [50, 128, 3001])
def test_summation_order(case, n):
    model = R.ellipsoid(n, seed=n)
    rng = np.random.default_rng(n)
    vals = rng.normal(size=(n, 5)) * 10.0 ** rng.integers(-6, 3, size=(n, 5))
    vals[rng.random(size=n) < 0.3] = 0.0   # lanes without a pair
    assert R.chunk_sums(vals).tobytes() == R.chunk_sums_loop(vals).tobytes()
    # the 28 sums of an evaluation, from the products a plain loop multiplies
    T = case["T"]
    depth = draw(model, T) if n != 3001 else case["depth"]
    T0 = R.offset_pose(T, case["centre"], [0.003, 0.0, 0.001], [0.0, 0.02, 0.0])
    c0 = R.centre(model, 1)
    tot, n_cons, n_pairs, ck = R.evaluate(model, T0, c0, depth, INTR, 0.02)
    assert n_pairs > 0 and n_cons >= n_pairs
    loop_tot, prods = R.evaluate_loop(model, T0, c0, depth, INTR, 0.02)   # the loop, shared with tests/test_refine_cases.py
    assert int((prods[:, 27] != 0).sum()) <= n_pairs
    assert tot.tobytes() == loop_tot.tobytes()
