"""The block cache's guard mode (ppf_debug_pool_guard / ppf_debug_pool_check) and every stage under it.

Without the guard a request is rounded up to a size class, so a store a few bytes past what a reserve() asked for lands in
slack nobody reads, and a reused block still holds the previous call's bytes, so a read of scratch nobody wrote sees
plausible data.  Under the guard a 0xA5 zone lies right in front of and right behind the bytes asked for, and fresh blocks
hold the word 0 (mode 1) or 1 (mode 2).  Here: the detector detects a planted write; every stage's own check helper (which
asserts the oracle's bytes) passes under both fill words with no zone damaged; and the same for requests whose size is
exactly a size class, the ones with no slack at all when the guard is off."""
import contextlib
import ctypes as C
import functools
import gc
import os

import numpy as np
import pytest

from yolo_ppf_pose_estimation_amd import _capi, synth
from yolo_ppf_pose_estimation_amd._capi import check, lib
from yolo_ppf_pose_estimation_amd.cloud_processor import DepthMap, DeviceCloud, Recognizer
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
from yolo_ppf_pose_estimation_amd.device import Workspace

pytestmark = pytest.mark.gpu

GOLDEN_BOTTLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bottle_model_xyzn.npy")
ZONE_CHECKED = 4096          # bytes of the back zone that are filled and checked (ppf_device_mem.h)
H2D, D2H = 1, 2              # hipMemcpyKind


@contextlib.contextmanager
def guard(mode):
    check(lib().ppf_debug_pool_guard(mode))
    try:
        yield
    finally:
        check(lib().ppf_debug_pool_guard(0))


def pool_check():
    """(the report, its violations as (requested_bytes, first_offset, n_bytes_damaged))"""
    r = _capi.PoolReport()
    check(lib().ppf_debug_pool_check(C.byref(r)))
    return r, [(int(v.requested_bytes), int(v.first_offset), int(v.n_bytes_damaged)) for v in r.first[:min(int(r.n_violations), 8)]]


@functools.lru_cache(maxsize=None)
def hip():
    """the process's HIP runtime: the one the library itself is linked to, found through the library's handle"""
    rt = C.CDLL(_capi.LIB_PATH)
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipMemcpy.restype = C.c_int
    return rt


def poke(address, data: bytes):
    assert hip().hipMemcpy(C.c_void_p(address), data, len(data), H2D) == 0


def test_arguments():
    assert lib().ppf_debug_pool_guard(3) == _capi.PPF_ERR_INVALID and lib().ppf_debug_pool_guard(-1) == _capi.PPF_ERR_INVALID
    assert lib().ppf_debug_pool_check(None) == _capi.PPF_ERR_INVALID


def test_the_detector_detects():
    rows = np.random.default_rng(1).uniform(-1, 1, size=(100, 6)).astype(np.float32)
    requested = 100 * 6 * 4                 # cloud_reserve: n x 6 floats
    zone = b"\xa5" * 4
    with guard(1):
        live = int(pool_check()[0].n_blocks_live)
        cloud = DeviceCloud.upload(rows)
        base, n = cloud.device_rows()
        assert n == 100 and base % 256 == 0
        r, v = pool_check()
        assert (r.n_blocks_live, r.n_violations) == (live + 2, 0) and r.n_blocks_checked >= 2      # the rows and the curvature
        assert cloud.rows().tobytes() == rows.tobytes()
        # a plain write inside the same allocation, just past what was asked for
        poke(base + requested, b"\x00\x00\x00\x00")
        r, v = pool_check()
        assert v == [(requested, requested, 4)], v
        poke(base + requested, zone)
        assert pool_check()[1] == []
        poke(base - 4, b"\x01\x02\x03\x04")
        assert pool_check()[1] == [(requested, -4, 4)]
        poke(base - 4, zone)
        poke(base + requested + ZONE_CHECKED - 1, b"\x00")       # the last checked byte
        assert pool_check()[1] == [(requested, requested + ZONE_CHECKED - 1, 1)]
        # released damaged: reported once more, from the release-time list, and then forgotten
        del cloud
        gc.collect()
        r, v = pool_check()
        assert v == [(requested, requested + ZONE_CHECKED - 1, 1)] and r.n_blocks_live == live
        assert pool_check()[1] == []
        # an untouched cloud, released, reports nothing; the block it reuses has its zones and fill again
        cloud = DeviceCloud.upload(rows)
        assert cloud.rows().tobytes() == rows.tobytes()
        del cloud
        gc.collect()
        r, v = pool_check()
        assert v == [] and r.n_blocks_checked >= 2 and r.n_blocks_live == live
    # a block acquired under the guard and released after it was switched off is still checked
    with guard(2):
        cloud = DeviceCloud.upload(rows)
        base, _ = cloud.device_rows()
    poke(base + requested, b"\x00\x00")
    del cloud
    gc.collect()
    with guard(1):
        assert pool_check()[1] == [(requested, requested, 2)]


def test_fill_words():
    """the usable bytes of a fresh block hold the mode's word: a cloud of no rows still reserves one row it never writes"""
    got = {}
    for mode in (1, 2):
        with guard(mode):
            cloud = DeviceCloud.upload(np.zeros((0, 6), np.float32))
            base, n = cloud.device_rows()
            assert n == 0
            words = (C.c_uint32 * 6)()
            assert hip().hipMemcpy(words, C.c_void_p(base), 24, D2H) == 0
            got[mode] = list(words)
            del cloud
            gc.collect()
            assert pool_check()[1] == []
    assert got == {1: [0] * 6, 2: [1] * 6}


# ---- every stage under the guard -----------------------------------------------------------------------------------------
def body(fixture):
    """the function behind a pytest fixture of another test file: what it keeps on the device is made when it is called"""
    return fixture.__wrapped__


def stage_parity(bottle):
    import test_gpu_parity as T
    scene, _ = synth.make_scene(bottle, n_points=5000, seed=21)
    T._check_against_oracle(PPF3DDetector(0.06, 0.05).trainModel(bottle), oracle_of(0.06), scene, 1.0 / 25.0, 0.05, True)


def stage_parity_two_tiles(bottle):
    import test_gpu_parity as T
    scene, _ = synth.make_scene(bottle, n_points=6000, seed=22)
    two = PPF3DDetector(0.036, 0.05, max_tile_refs=1000).trainModel(bottle)
    assert two.info()["n_tiles"] == 2
    T._check_against_oracle(two, oracle_of(0.036), scene, 1.0 / 100.0, 0.05, True)


@functools.lru_cache(maxsize=None)
def oracle_of(step):
    import oracle_lib as O
    return O.OracleDetector(step, 0.05).train_model(np.load(GOLDEN_BOTTLE))


@functools.lru_cache(maxsize=None)
def accumulator_case():
    """one scene for test_gpu_accumulators' check: the bottle at 430 presampled rows, 3,000 scene rows, every 500th a reference
    point (host side only: the oracle and the cache of its accumulators, computed once)"""
    import oracle_lib as O
    import test_gpu_accumulators as A
    bottle = np.load(GOLDEN_BOTTLE)
    rows = O.OracleDetector(A.SAMPLING, A.DISTANCE).train_model(bottle).sampled_model()
    ora = O.OracleDetector(A.SAMPLING, A.DISTANCE).train_model(rows, presampled=True)
    scene = synth.make_scene(bottle, n_points=A.N_SCENE, seed=31)[0].astype(np.float32)
    return rows, ora, scene, list(range(0, A.N_SCENE, 500)), {}


def stage_accumulators(bottle):
    import test_gpu_accumulators as A
    rows, ora, scene, refs, want = accumulator_case()
    det = PPF3DDetector(A.SAMPLING, A.DISTANCE).trainModel(rows, presampled=True)
    for acc32 in (0, 1):
        ws = Workspace()
        ws.set_option(_capi.PPF_OPT_ACC32, acc32)
        st = A.check(ws, det, ora, scene, 1.0, refs, want, ref_stride=500, vote_mode=0)
        assert (st["n_acc32_items"] > 0) == bool(acc32) and st["n_votes"] > 0


stage_accumulators.prepare = accumulator_case      # host work, done before the guard is on


def stage_icp(bottle):
    import test_gpu_icp as T
    P = synth.rigid_pose(5, 0.1)
    model, scene = bottle[::8].copy(), synth.apply_pose(bottle[3::5], P)
    T._check(model, scene, [T._perturb(P, 4.0, [0.004, -0.003, 0.002]), T._perturb(P, -3.0, [0.0, 0.002, 0.001], axis=0), P])


def stage_cloud_stages(bottle):
    import prep_data as D
    import test_gpu_prep as T
    T.test_stages_random_draw(D.c1_frame(), 1)      # draw 1: the synthetic plane + sphere cloud, never an empty window


def stage_planes(bottle):
    import test_gpu_planes as T
    T.check([T.mixed(65, seed=1), T.mixed(257, seed=2)], T.SMALL)


def stage_clusters(bottle):
    import test_gpu_clusters as T
    T.check([T.scattered(65, seed=1), T.scattered(257, seed=2)], dict(T.SMALL, max_clusters=256))


def stage_regions(bottle):
    import region_cases as RC
    import test_gpu_regions as T
    T.check([RC.patches(65, seed=1), RC.patches(257, seed=2)], dict(T.SMALL, tolerance=0.02))


def stage_cloud_from_depth(bottle):
    import test_gpu_depth as T
    rng = np.random.default_rng(5)
    intr = (610.0, 608.0, 99.5, 17.25)
    assert T.check_equal(T.make_image(rng, (37, 200), 0.5, np.float32), intr) > 0
    assert T.check_equal(T.make_image(rng, (37, 200), 0.5, np.uint16), intr, depth_scale=0.001, fp64=True) > 0


def stage_cloud_from_depth_normals(bottle):
    import test_gpu_depth_normals as T
    rng = np.random.default_rng(6)
    intr = (610.0, 608.0, 99.5, 17.25)
    T.check_equal(T.surface(rng, (37, 200), 0.9), intr, fp64=True)
    T.check_equal(T.surface(rng, (37, 200), 0.9, dtype=np.uint16), intr, depth_scale=0.001, drop=True)


def stage_depth_filter(bottle):
    import test_gpu_depth_filter as T
    rng = np.random.default_rng(7)
    _, counts = T.check_equal(T.seeded(rng, (37, 200)))
    assert counts["n_unsupported"] > 0 and counts["n_written"] > 0
    T.check_equal(T.seeded(rng, (37, 200), dtype=np.uint16), radius=2)


def stage_depth_segments(bottle):
    import depth_segments_oracle as S
    import test_gpu_depth_segments as T
    rng = np.random.default_rng(8)
    for shape in ((17, 65), (33, 129)):
        img = T.seeded(rng, shape)
        nrm = T.seeded_normals(rng, img)
        for flags in (0, S.EIGHT):
            T.check_equal(img, min_size=1, flags=flags)
            T.check_equal(img, normals=nrm, min_size=1, max_segments=256, flags=flags)


def stage_depth_history(bottle):
    import test_gpu_depth_history as T
    rng = np.random.default_rng(9)
    for shape in ((5, 65), (9, 129)):
        for window, kw in ((3, {}), (16, dict(mean=True, max_age=15))):
            T.check_sequence(T.sequence(rng, shape, 2 * window + 2), window=window, **kw)       # the ring wraps
    T.check_sequence(T.sequence(rng, (5, 65), 8, dtype=np.uint16), window=3, mean=True, min_support=2)


def stage_depth_register(bottle):
    import register_oracle as O
    import test_gpu_register as T
    cam = T.small_depth_cam(18, 33)
    m = DepthMap(cam, (18, 33), T.CCAM, (T.CROWS, T.CCOLS), T.R, T.T)
    _, st = T.check(m, O.plane_depth(cam, 18, 33), cam, T.CCAM, (T.CROWS, T.CCOLS))
    assert st["n_filled"] > 0


def stage_depth_motion(bottle):
    import test_gpu_depth_motion as T
    for rows, cols in ((25, 41), (66, 130)):
        prev, cur, intr, _, want = T.sized(rows, cols)
        T.same(T.device(prev, cur, intr), want, (rows, cols))


def stage_match_frame(bottle):
    import test_gpu_match_frame as T
    pairs, (db, cb), (ds, cs), mp = body(T.rendered)(bottle)
    rows, _, st = T.check_against_loop([(db, cb, pairs[0][0], pairs[0][1]), (ds, cs, pairs[2][0], pairs[2][1])], mp, T.icp_params(), 5)
    assert rows[0] and rows[1] and st.n_dets == 2


def stage_verify(bottle):
    import test_gpu_verify as T
    c1 = body(T.c1)(bottle)
    _, _, st = T.check_parity([bottle], [c1["obj_rows"]], [c1["poses"]], T.params(), c1["depth"], c1["intr"], [(c1["mcloud"], c1["obj"])])
    assert st["n_jobs"] == 5


def stage_render(bottle):
    import test_gpu_render as T
    c1 = body(T.c1)(bottle)
    shape, intr = c1["depth"].shape, c1["intr"]
    _, _, st = T.check_rendered([bottle], [c1["obj_rows"]], [(c1["mcloud"], c1["obj"])], [c1["poses"][:2]], T.params(), T.RP, shape, intr,
                                c1["depth"])
    assert st["n_jobs"] == 2
    got = T.render_frame([c1["mcloud"]] * 2, [c1["poses"][:2]] * 2, [0, 1], shape[0], shape[1], intr, T.RP)
    T.assert_images(got, T.frame_oracle([(bottle, c1["poses"][k]) for k in range(2)], shape, intr, T.RP["splat_radius"]))


def stage_select(bottle):
    import test_gpu_select as T
    c1 = body(T.c1)(bottle)
    poses = [[P] for P in c1["poses"][:3]]
    T.check_select([bottle] * 3, [c1["mcloud"]] * 3, poses, c1["depth"], c1["intr"], T.RP, dict(max_overlap=0.25, depth_tol=0.01, min_pixels=1),
                   None, 1, c1["cache"])


def stage_refine(bottle):
    import refine_oracle as R
    import test_gpu_refine as T
    case = body(T.case)()
    poses = [case["poses"][0][:2], case["poses"][1][:2]]
    mats, info, st, _ = T.call(case["clouds"][:2], poses, case["depth"], T.INTR)
    assert st["n_jobs"] == 4 and st["n_launches"] == 1
    for i in range(2):
        for k in range(2):
            P, want = R.refine(case["models"][i], poses[i][k], case["depth"], T.INTR, {})
            T.assert_job(mats[i, k], info[i, k], P, want, (i, k))


def stage_recognize(bottle):
    import recognize_cases as K
    import recognize_oracle as R
    import test_gpu_recognize as T
    dets = [T.train(*m) for m in T.MODELS[:2]]
    rec = Recognizer(dets)
    views = [K.thin(K.one_sided_view(T.full_cloud(kind), 40 + i), n, seed=n) for i, (kind, n) in enumerate((("box", 65), ("cylinder", 63)))]
    T.check_call(rec, [R.Model.from_detector(d) for d in dets], views + [None], top=2)


STAGES = [stage_parity, stage_parity_two_tiles, stage_accumulators, stage_icp, stage_cloud_stages, stage_planes, stage_clusters,
          stage_regions, stage_cloud_from_depth, stage_cloud_from_depth_normals, stage_depth_filter, stage_depth_segments,
          stage_depth_history, stage_depth_register, stage_depth_motion, stage_match_frame, stage_verify, stage_render, stage_select,
          stage_refine, stage_recognize]


def run_guarded(mode, fn, *args):
    """fn under the guard: everything it made is released inside the guarded section, then no zone may be damaged"""
    with guard(mode):
        pool_check()
        try:
            fn(*args)
        finally:
            gc.collect()
        r, v = pool_check()
        assert r.n_violations == 0, (fn.__name__, mode, int(r.n_violations), v)
        assert r.n_blocks_checked > 0, "the stage drew nothing from the block cache"


@pytest.mark.parametrize("stage", STAGES, ids=[s.__name__[6:] for s in STAGES])
def test_stage_under_the_guard(stage, bottle):
    """the stage's own helper asserts the oracle's bytes: equal under the fill words 0 and 1 means nothing read was stale"""
    getattr(stage, "prepare", lambda: None)()
    for mode in (1, 2):
        run_guarded(mode, stage, bottle)


# ---- request sizes on a class boundary -------------------------------------------------------------------------------------
def on_a_class(n_bytes):
    """the request is its own block: without the guard there is no slack behind it"""
    return lib().ppf_debug_block_size(n_bytes) == n_bytes


def test_history_ring_on_a_class_boundary():
    import test_gpu_depth_history as T
    # the ring: window planes of rows x 4 ceil(cols / 4) floats.  4 x (9 x 64) x 4 B = 9,216 B = 9 << 10;
    # 3 x (10 x 64) x 4 B = 7,680 B = 15 << 9 with cols 61..64 (the plane is padded to 64)
    rng = np.random.default_rng(10)
    for (rows, cols), window in (((9, 64), 4), ((10, 61), 3)):
        assert rows * cols < 40000 and on_a_class(window * rows * ((cols + 3) // 4 * 4) * 4)
        run_guarded(2, lambda: T.check_sequence(T.sequence(rng, (rows, cols), 2 * window + 2), window=window))
    assert on_a_class(9 * 64 * 4) and on_a_class(9 * 64)       # 9 x 64: also the fused image and the state the host entry stages


def test_depth_uploads_on_a_class_boundary():
    import test_gpu_depth as Dp
    import test_gpu_depth_filter as Df
    import test_gpu_depth_normals as Dn
    # 24 x 80 pixels: 7,680 B = 15 << 9 as float32, 3,840 B = 15 << 8 as uint16; 80 columns end inside a 64-wide tile
    shape = (24, 80)
    assert shape[0] * shape[1] < 40000 and on_a_class(24 * 80 * 4) and on_a_class(24 * 80 * 2)
    rng = np.random.default_rng(11)
    intr = (610.0, 608.0, 39.5, 11.25)

    def case():
        assert Dp.check_equal(Dp.make_image(rng, shape, 0.5, np.float32), intr) > 0
        assert Dp.check_equal(Dp.make_image(rng, shape, 0.5, np.uint16), intr, depth_scale=0.001) > 0
        Dn.check_equal(Dn.surface(rng, shape, 0.9), intr, fp64=True)
        Dn.check_equal(Dn.surface(rng, shape, 0.9, dtype=np.uint16), intr, depth_scale=0.001)
        Df.check_equal(Df.seeded(rng, shape))
        Df.check_equal(Df.seeded(rng, shape, dtype=np.uint16), radius=2)
    run_guarded(2, case)


def test_segment_arrays_on_a_class_boundary():
    import depth_segments_oracle as S
    import test_gpu_depth_segments as T
    # an int32 or a float per pixel: 24 x 80 x 4 B = 7,680 B = 15 << 9, and 40 x 96 x 4 B = 15,360 B = 15 << 10, which has more than
    # one 64 x 16 tile in both directions
    rng = np.random.default_rng(12)
    for shape in ((24, 80), (40, 96)):
        assert on_a_class(shape[0] * shape[1] * 4)
        img = T.seeded(rng, shape)
        nrm = T.seeded_normals(rng, img)

        def case():
            T.check_equal(img, min_size=1)
            T.check_equal(img, normals=nrm, min_size=1, max_segments=256, flags=S.EIGHT)
        run_guarded(2, case)
