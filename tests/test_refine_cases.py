"""The cases of tests/refine_cases.py on the CPU, against tests/refine_oracle.py: every case reaches what it is there for (its
condition, and the counts worked out by hand), the oracle's 28 sums are those of a plain loop over the rows, and
the cases tell the rules of DESIGN.md §17 apart: every mutant of refine_oracle.MUTANTS changes the bytes of a case that pins
its rule.  tests/test_gpu_refine.py holds the device to the same cases."""
import numpy as np
import pytest

import refine_cases as RC
import refine_oracle as R

_SPEC = {}


def outcome(c, mutant=None):
    """[(run, model, pose, T, info, trace)] of every pose of the case"""
    out = []
    for r, i, k in RC.jobs(c):
        trace = []
        T, info = R.refine(r["models"][i], r["poses"][i][k], r["depth"], r["intr"], r["prm"], mutant, trace)
        out.append((r, i, k, T, info, trace))
    return out


def spec(name):
    if name not in _SPEC:
        _SPEC[name] = outcome(RC.old_fixture() if name == "old fixture" else RC.case(name))
    return _SPEC[name]


def job_bytes(job):
    _, _, _, T, info, _ = job
    return T.tobytes() + b"".join(np.asarray(info[f]).tobytes() for f in R.INFO_FIELDS)


def by_run(name, what):
    return [j for j in spec(name) if j[0]["what"] == what]


def went(job, status, iterations=None):
    info = job[4]
    return info["status"] == status and (iterations is None or info["iterations"] == iterations)


def unmoved(job):
    r, i, k, T, info, _ = job
    return info["iterations"] == 0 and T.tobytes() == np.asarray(r["poses"][i][k], dtype=np.float64).tobytes()


# ---- 1. the conditions and the hand counts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.NAMES)
def test_hand_counts(name):
    """what refine_cases.py worked out by hand is what the oracle reports"""
    for r, i, k, T, info, _ in spec(name):
        for f, v in r["hand"].get((i, k), {}).items():
            assert info[f] == v, (name, r["what"], i, k, f, info)


def test_lattice():
    want = {(16, False): 1024, (11, False): 704, (16, True): 512, (11, True): 352}
    half_even = {(16, True): 640, (11, True): 472}
    truncated = {(16, True): 545, (11, True): 381}
    for job in spec("lattice"):
        r, _, _, T, info, _ = job
        key = (r["depth"].shape[0], bool((r["depth"] == 0).any()))
        assert RC.lattice_pairs(key[0], 16, key[1]) == want[key] == info["n_pairs_first"]
        assert went(job, R.CONVERGED, 1) and info["n_considered"] == 1369 and T.tobytes() == np.eye(4).tobytes()
        if key[1]:   # the checkerboard tells the roundings apart
            assert RC.lattice_pairs(key[0], 16, True, lambda x: int(np.rint(x))) == half_even[key] != want[key]
            assert RC.lattice_pairs(key[0], 16, True, lambda x: int(x + 0.5)) == truncated[key] != want[key]


def test_holes():
    c = RC.case("holes")
    r = c["runs"][0]
    assert (r["depth"] == 0).any() and np.isnan(r["depth"]).any() and np.isinf(r["depth"]).any() and (r["depth"] < 0).any()
    for job in spec("holes"):
        _, i, k, _, info, _ = job
        whole = R.evaluate(r["models"][i], r["poses"][i][k], R.centre(r["models"][i], 1), c["whole"], r["intr"], 0.02)[2]
        print(f"start {k}: {whole} pairs on the whole image, {info['n_pairs_first']} with holes, status {info['status']}")
        assert info["n_pairs_first"] <= 0.85 * whole, (k, whole, info)
        assert info["status"] in (R.CONVERGED, R.MAX_ITERS) and info["iterations"] > 0, (k, info)
    assert (spec("holes")[0][4]["n_pairs_first"], R.evaluate(r["models"][0], r["poses"][0][0], R.centre(r["models"][0], 1), c["whole"], r["intr"], 0.02)[2]) == (1054, 1286)


def outside_share(model, T, rows, cols, intr):
    """of the considered rows of the pose, the share whose pixel is outside the image"""
    fx, fy, ppx, ppy = intr
    o = R.transform_rows(model, T).astype(np.float64)
    cons = np.isfinite(o).all(axis=1) & ((o[:, 3] * o[:, 0] + o[:, 4] * o[:, 1]) + o[:, 5] * o[:, 2] < 0)
    assert (o[cons, 2] > 0).all()
    ui, vi = np.floor(o[:, 0] * fx / o[:, 2] + ppx + 0.5), np.floor(o[:, 1] * fy / o[:, 2] + ppy + 0.5)
    out = cons & ~((ui >= 0) & (ui < cols) & (vi >= 0) & (vi < rows))
    return out.sum() / cons.sum()


def test_borders():
    sides = set()
    for job in spec("borders"):
        r, i, k, _, info, trace = job
        shares = [outside_share(r["models"][i], T, *r["depth"].shape, r["intr"]) for T, _, _ in trace]
        print(r["what"], info["n_considered"], info["n_pairs_first"], info["n_pairs_last"], [round(float(s), 3) for s in shares])
        assert len(trace) == info["iterations"] and all(0.3 <= s <= 0.7 for s in shares), (r["what"], shares)
        assert went(job, R.CONVERGED) and 544 <= info["n_pairs_last"] <= 752 and 1300 <= info["n_considered"] <= 1420, (r["what"], info)
        sides.add(r["what"])
    assert sides == {"left", "right", "top", "bottom", "corner"}


def test_shell():
    c = RC.case("shell")
    model = c["runs"][0]["models"][0]
    assert int((R.transform_rows(model, c["T"])[:, 2] <= 0).sum()) == 1321 and len(model) == 3001
    for job in by_run("shell", "share 0.1"):
        assert went(job, R.CONVERGED) and job[4]["n_considered"] == 3001 and 570 <= job[4]["n_pairs_last"] <= 600, job[4]
    for job in by_run("shell", "default share"):   # the share guard fires while min_pairs does not
        info = job[4]
        assert went(job, R.LOST, 0) and unmoved(job) and 577 <= info["n_pairs_first"] <= 591 and info["n_pairs_first"] >= R.DEFAULTS["min_pairs"]
        assert info["n_pairs_first"] < R.DEFAULTS["min_pair_share"] * info["n_considered"]


def test_bad_rows():
    c = RC.case("bad_rows")
    assert int((~np.isfinite(c["bad"]).all(axis=1)).sum()) == 300
    assert R.centre(c["bad"], 1).tobytes() != R.centre(c["clean"], 1).tobytes() and np.isfinite(R.centre(c["bad"], 1)).all()
    assert R.centre(np.full((130, 6), np.nan, np.float32), 1).tobytes() == np.zeros(3).tobytes()
    jobs = spec("bad_rows")
    assert went(jobs[0], R.CONVERGED) and jobs[0][4]["n_rows"] == 3001
    for job in jobs[1:]:
        assert went(job, R.LOST, 0) and unmoved(job) and job[4]["n_considered"] == 0, job[4]
    assert not np.isfinite(jobs[2][3]).all() and not np.isfinite(jobs[3][3]).all()


def test_plane_sizes_limits_intrinsics():
    exact, deeper, tilted = by_run("plane", "exact, 4 mm deeper, tilted")
    assert went(exact, R.CONVERGED, 1) and went(deeper, R.CONVERGED, 2) and went(tilted, R.CONVERGED, 3)
    assert went(by_run("plane", "tilted, eps 0, 100 iterations")[0], R.MAX_ITERS, 100)
    assert went(by_run("plane", "tied pivots, one step")[0], R.MAX_ITERS, 1)
    big = by_run("sizes", "4,096, 4,097 and 38,209 rows, then 6 and 16")
    assert [j[4]["n_rows"] for j in big] == [4096, 4097, 38209, 6, 16]
    assert went(big[0], R.CONVERGED, 8) and went(big[1], R.CONVERGED, 6) and went(big[2], R.CONVERGED, 7)
    step9 = by_run("sizes", "38,209 rows, model_step 9")[0]
    assert step9[4]["n_rows"] == 4246 and went(step9, R.CONVERGED)
    cuts = by_run("sizes", "1, 6, 15, 16, 63, 64 and 65 rows")
    assert [j[4]["n_rows"] for j in cuts] == [1, 6, 15, 16, 63, 64, 65] and went(cuts[0], R.LOST, 0)
    assert went(by_run("sizes", "128 rows, eps 0, 100 iterations")[0], R.MAX_ITERS, 100)
    lim = spec("limits")[0]
    assert went(lim, R.STEP, 0) and unmoved(lim) and lim[4]["n_pairs_first"] == lim[4]["n_pairs_last"] > 1000
    odd, flipped = spec("intrinsics")
    assert odd[0]["depth"].shape == (97, 131) and odd[4]["status"] in (R.CONVERGED, R.MAX_ITERS) and odd[4]["iterations"] > 0
    assert flipped[0]["intr"][1] < 0 and went(flipped, R.CONVERGED, 7)


def test_every_status_is_reached_by_a_new_case():
    seen = {}
    for name in RC.NAMES:
        for job in spec(name):
            seen.setdefault(int(job[4]["status"]), name)
    assert set(seen) == {R.CONVERGED, R.MAX_ITERS, R.LOST, R.STEP}, seen   # NONE is a row without a pose: the device test has one


def test_random_draws_are_what_they_say():
    """the draws of tests/test_gpu_refine.py::test_refine_random_draw: within their ranges, and between them some pose moves"""
    moved = 0
    for seed in range(6):
        cfg, r = RC.random_draw(seed)
        rows, cols = r["depth"].shape
        assert rows % 2 == cols % 2 == 1 and rows <= 120 and cols <= 160 and r["intr"][0] != r["intr"][1]
        assert 1 <= len(r["models"][0]) <= 5000 and 1 <= r["prm"]["model_step"] <= 7 and 1 <= len(r["poses"][0]) <= 4
        assert 0 <= cfg["holes"] <= 0.4 and cfg["gate"] in (0.005, 0.01, 0.02) and all(mm <= 12 and deg <= 6 for mm, deg in cfg["starts"])
        moved += sum(R.refine(r["models"][0], T, r["depth"], r["intr"], r["prm"])[1]["iterations"] > 0 for T in r["poses"][0])
    assert moved >= 6


# ---- 2. a second source for the sums ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.NAMES)
def test_first_evaluation_sums_by_a_plain_loop(name):
    """the 28 sums of the first evaluation of every (run, model): refine_oracle.evaluate against the per-row loop"""
    n_pairs = 0
    for r in RC.case(name)["runs"]:
        step = r["prm"].get("model_step", 1)
        gate = r["prm"].get("depth_gate", R.DEFAULTS["depth_gate"])
        for model, plist in zip(r["models"], r["poses"]):
            c0 = R.centre(model, step)
            tot, _, n, _ = R.evaluate(model[::step], plist[0], c0, r["depth"], r["intr"], gate)
            loop_tot, prods = R.evaluate_loop(model[::step], plist[0], c0, r["depth"], r["intr"], gate)
            assert tot.tobytes() == loop_tot.tobytes(), (name, r["what"], len(model))
            assert int(prods.any(axis=1).sum()) <= n
            n_pairs += n
    assert n_pairs > 0


# ---- 3. the mutants ----------------------------------------------------------------------------------------------------------------
OLD_FIXTURE_CATCHES = {"min_pairs_le", "chunks_reversed"}   # the record: what tests/test_gpu_refine.py::case told apart before these cases


def test_every_pinned_rule_has_a_mutant():
    pinned = {rule for name in RC.NAMES for rule in RC.case(name)["pins"]}
    assert pinned == {rule for rule, _ in R.MUTANTS.values()}


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutant_changes_a_case_that_pins_its_rule(mutant):
    rule, what = R.MUTANTS[mutant]
    changed = {}
    for name in RC.NAMES:
        if rule in RC.case(name)["pins"]:
            got = outcome(RC.case(name), mutant)
            changed[name] = sum(job_bytes(a) != job_bytes(b) for a, b in zip(got, spec(name)))
    old = sum(job_bytes(a) != job_bytes(b) for a, b in zip(outcome(RC.old_fixture(), mutant), spec("old fixture")))
    print(f"{mutant} ({what}): poses changed per case {changed}; of the old fixture {old} of {len(spec('old fixture'))}")
    assert changed and any(changed.values()), (mutant, changed)
    assert (old > 0) == (mutant in OLD_FIXTURE_CATCHES), (mutant, old)


class Guarded(np.ndarray):
    """a depth image that refuses an index outside itself (numpy would wrap a negative one)"""

    def __getitem__(self, idx):
        if isinstance(idx, tuple) and len(idx) == 2 and all(isinstance(a, np.ndarray) for a in idx):
            assert all(((a >= 0) & (a < n)).all() for a, n in zip(idx, self.shape)), idx
        return np.asarray(self).__getitem__(idx)


@pytest.mark.parametrize("mutant", [None] + list(R.MUTANTS))
def test_no_mutant_reads_outside_the_image(mutant):
    for name in ("lattice", "near_zero", "borders", "shell", "bad_rows"):
        for r in RC.case(name)["runs"]:
            for model, plist in zip(r["models"], r["poses"]):
                for T in plist:
                    R.evaluate(model, T, R.centre(model, 1, mutant), r["depth"].view(Guarded), r["intr"], 0.02, mutant)
