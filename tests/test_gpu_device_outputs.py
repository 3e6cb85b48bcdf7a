"""Nothing outside a caller's device buffer is written.  The device entries that write into memory the caller owns get their
output inside a larger arena that is filled with a canary: ``pre`` elements in front, the output window, 64 elements behind.
After the call the window holds the oracle's bytes and every other element of the arena still holds the canary.  ``pre`` also
moves the window off the alignment a fresh allocation has, which takes the element-store paths of the kernels that write
vectors when the pointer allows it (k_history_push's out and state, the stores at a row's tail)."""
import ctypes as C

import numpy as np
import pytest

import depth_filter_oracle as F
import depth_history_oracle as H
import depth_segments_oracle as S
import register_oracle as RO
from test_depth_filter_oracle import seeded
from test_depth_history_oracle import sequence
from yolo_ppf_pose_estimation_amd import _capi, synth
from yolo_ppf_pose_estimation_amd._capi import Pose, check, lib
from yolo_ppf_pose_estimation_amd.cloud_processor import DepthHistory, DepthMap, filter_depth, segment_depth
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector
from yolo_ppf_pose_estimation_amd.device import BatchMatcher, Workspace

pytestmark = pytest.mark.gpu

CANARY32 = 0x7FC0A5A5      # as a float: a NaN no stage writes
CANARY8 = 0xA5
BEHIND = 64


class Arena:
    """`pre` canary elements, a window of `n`, BEHIND canary elements; int32 (for float and label outputs) or uint8"""

    def __init__(self, pre, n, dtype=np.int32):
        import torch
        self.pre, self.n = pre, n
        self.canary = CANARY32 if dtype == np.int32 else CANARY8
        self.mem = torch.full((pre + n + BEHIND,), self.canary, dtype=torch.int32 if dtype == np.int32 else torch.uint8, device="cuda")

    def refill(self):
        self.mem.fill_(self.canary)

    @property
    def ptr(self):
        return self.mem.data_ptr() + self.pre * self.mem.element_size()

    def view(self, torch_dtype, shape):
        """the window as a tensor an ``out=`` argument takes"""
        return self.mem.view(torch_dtype)[self.pre:self.pre + self.n].view(shape)

    def check(self, want, what):
        """the window holds want's bytes, everything around it the canary"""
        got = self.mem.cpu().numpy()
        win = got[self.pre:self.pre + self.n]
        w = np.ascontiguousarray(want).reshape(-1).view(win.dtype)
        assert w.size == self.n
        assert (got[:self.pre] == self.canary).all(), (what, "written in front of the output", np.flatnonzero(got[:self.pre] != self.canary))
        tail = got[self.pre + self.n:]
        assert (tail == self.canary).all(), (what, "written behind the output", np.flatnonzero(tail != self.canary))
        if win.tobytes() != w.tobytes():
            bad = np.flatnonzero(win != w)
            raise AssertionError(f"{what}: {bad.size} elements differ from the oracle, first {bad[0]}: {int(win[bad[0]]):#x} against {int(w[bad[0]]):#x}")


# ---- ppf_depth_history_push_device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [60, 61, 63, 64])
def test_history_push_device_writes_only_its_outputs(cols):
    """out at 0..3 floats and state at 0..3 bytes past an aligned address, every pair of the two: with cols 60 and 64 an
    aligned pointer takes the vector stores and a misaligned one the element stores of a row that would allow vectors"""
    import torch
    shape, window, pushes = (9, cols), 4, 6
    n = shape[0] * shape[1]
    rng = np.random.default_rng(600 + cols)
    for dtype in (np.float32, np.uint16):
        frames = sequence(rng, shape, pushes, dtype=dtype)
        ora = H.History(window=window, mean=dtype == np.uint16)
        want = [ora.push(f) for f in frames]
        dev = [torch.from_numpy(f).cuda() for f in frames]
        for pre_out in range(4):
            for pre_state in range(4):
                out, state = Arena(pre_out, n), Arena(pre_state, n, np.uint8)
                assert out.ptr % 16 == 4 * pre_out and state.ptr % 4 == pre_state
                h = DepthHistory(shape, dtype=dtype, params=dict(window=window, flags=_capi.PPF_HISTORY_MEAN if dtype == np.uint16 else 0))
                for t in range(pushes):
                    out.refill()
                    state.refill()
                    st = _capi.DepthHistoryStats()
                    check(lib().ppf_depth_history_push_device(h._ptr, C.c_void_p(dev[t].data_ptr()), cols * frames[t].itemsize, C.c_void_p(out.ptr),
                                                              C.c_void_p(state.ptr), None, C.byref(st)))
                    what = f"{dtype.__name__} cols {cols} out +{pre_out} state +{pre_state} push {t}"
                    out.check(want[t][0], what + " out")
                    state.check(want[t][1], what + " state")
                    assert {k: getattr(st, k) for k in H.COUNTS} == want[t][2], what


# ---- ppf_depth_filter_device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [63, 64, 65])
def test_depth_filter_device_writes_only_its_output(cols):
    """both sides of the 64-wide tile, five rows: the last tile row is partial"""
    import torch
    shape = (5, cols)
    rng = np.random.default_rng(700 + cols)
    for dtype in (np.float32, np.uint16):
        img = seeded(rng, shape, dtype=dtype)
        want, counts = F.filter_depth(img)
        for pre in (0, 1, 3):
            a = Arena(pre, img.size)
            got, st = filter_depth(torch.from_numpy(img).cuda(), out=a.view(torch.float32, shape), return_stats=True)
            assert got.data_ptr() == a.ptr and {k: st[k] for k in counts} == counts
            a.check(want, f"filter {dtype.__name__} cols {cols} +{pre}")


# ---- ppf_depth_segments_device ----------------------------------------------------------------------------------------------
def test_depth_segments_device_writes_only_its_labels():
    import torch
    shape = (17, 65)
    rng = np.random.default_rng(800)
    img = seeded(rng, shape)
    for flags in (0, S.EIGHT):
        want = S.segments(img, min_size=1, flags=flags)[0]
        assert want.max() > 0
        for pre in (0, 1, 3):
            a = Arena(pre, img.size)
            got = segment_depth(torch.from_numpy(img).cuda(), params=dict(min_size=1, flags=flags), out=a.view(torch.int32, shape))
            assert got.data_ptr() == a.ptr
            a.check(want, f"segments flags {flags} +{pre}")


# ---- ppf_depth_register_device ----------------------------------------------------------------------------------------------
def test_depth_register_device_writes_only_its_image():
    """a 90 x 120 colour image (no multiple of the 16-pixel tile in either direction) from an 18 x 33 depth image"""
    import torch
    from test_gpu_register import CCAM, CCOLS, CROWS, R, T, small_depth_cam
    assert CROWS % 16 and CCOLS % 16
    cam = small_depth_cam(18, 33)
    depth = RO.plane_depth(cam, 18, 33)
    want, cnt, _ = RO.register(np.ascontiguousarray(depth), cam, CCAM, CROWS, CCOLS, R, T)
    assert cnt["n_filled"] > 0
    m = DepthMap(cam, (18, 33), CCAM, (CROWS, CCOLS), R, T)
    for pre in (0, 1, 3):
        a = Arena(pre, CROWS * CCOLS)
        got, st = m.register(torch.from_numpy(depth).cuda(), out=a.view(torch.float32, (CROWS, CCOLS)), return_stats=True)
        assert got.data_ptr() == a.ptr and {k: st[k] for k in cnt} == cnt
        a.check(want, f"register +{pre}")


# ---- pose blocks ------------------------------------------------------------------------------------------------------------
ROW = C.sizeof(Pose) // 4     # a pose record in int32 words


def pose_arena(pre_rows, rows):
    return Arena(pre_rows * ROW, rows * ROW)


def record_bytes(records, k, n):
    """the first min(k, n) records, then zero rows up to k"""
    raw = b"".join(bytes(records[i]) for i in range(min(k, n)))
    return np.frombuffer(raw + bytes((k - min(k, n)) * C.sizeof(Pose)), dtype=np.int32)


@pytest.fixture(scope="module")
def matched(bottle):
    """one match on a workspace: (workspace, the host route's per-reference records, n_ref, its clustered records, n_poses)"""
    import torch
    det = PPF3DDetector(0.06, 0.05).trainModel(bottle)
    scene, _ = synth.make_scene(bottle, n_points=3000, seed=31)
    d_scene = torch.from_numpy(np.ascontiguousarray(scene, dtype=np.float32)).cuda()
    ws = Workspace()
    ws.match_device(det, d_scene.data_ptr(), scene.shape[0], 6, 1.0 / 25.0, 0.05)
    cap = scene.shape[0]
    raw, fin = (Pose * cap)(), (Pose * cap)()
    n_ref, n_pose = C.c_int(0), C.c_int(0)
    check(lib().ppf_workspace_results(ws.ptr, None, raw, cap, C.byref(n_ref), fin, cap, C.byref(n_pose), None))
    assert n_ref.value == 120 and n_pose.value >= 2
    return dict(ws=ws, det=det, scene=d_scene, raw=raw, n_ref=n_ref.value, fin=fin, n_poses=n_pose.value)


def test_copy_top_poses_writes_k_records(matched):
    import torch
    n = matched["n_poses"]
    for k in sorted({1, n - 1, n, n + 1, n + 7}):
        for pre in (0, 1):
            a = pose_arena(pre, k)
            check(lib().ppf_workspace_copy_top_poses(matched["ws"].ptr, C.c_void_p(a.ptr), k, None))
            torch.cuda.synchronize()
            a.check(record_bytes(matched["fin"], k, n), f"top poses k {k} of {n} +{pre}")


def test_copy_raw_poses_writes_cap_records(matched):
    import torch
    n = matched["n_ref"]
    for cap in (n, n + 1, n + 9):
        for pre in (0, 1):
            a = pose_arena(pre, cap)
            check(lib().ppf_workspace_copy_raw_poses(matched["ws"].ptr, C.c_void_p(a.ptr), cap, None))
            torch.cuda.synchronize()
            a.check(record_bytes(matched["raw"], cap, n), f"raw poses cap {cap} of {n} +{pre}")
    # below the count: refused, nothing written
    a = pose_arena(1, n - 1)
    assert lib().ppf_workspace_copy_raw_poses(matched["ws"].ptr, C.c_void_p(a.ptr), n - 1, None) == _capi.PPF_ERR_CAPACITY
    torch.cuda.synchronize()
    assert (a.mem.cpu().numpy() == CANARY32).all()


def test_batch_copy_block_writes_n_records(matched):
    import torch
    top_k, crops = 3, 2
    bm = BatchMatcher(lanes=2)
    det = matched["det"]
    models = (C.c_void_p * 1)(det._model.ptr)
    scenes = (C.c_void_p * crops)(*[matched["scene"].data_ptr()] * crops)
    counts = (C.c_int * crops)(3000, 1500)
    mp = det._params(1.0 / 25.0, 0.05, True)
    out, n_out, st = (Pose * (crops * top_k))(), (C.c_int * crops)(), _capi.BatchStats()
    check(lib().ppf_batch_run(bm.ptr, models, 1, scenes, counts, 6, 3, crops, 1, C.byref(mp), out, top_k, n_out, C.byref(st)))
    records = crops * top_k
    assert max(n_out) > 0
    # the host route's bytes: each crop's records, then zero rows up to top_k
    want = np.concatenate([record_bytes([out[c * top_k + i] for i in range(top_k)], top_k, n_out[c]) for c in range(crops)])
    for n in (1, records - 1, records):
        for pre in (0, 1):
            a = pose_arena(pre, n)
            check(lib().ppf_batch_copy_block(bm.ptr, C.c_void_p(a.ptr), n, None))
            torch.cuda.synchronize()
            a.check(want[:n * ROW], f"batch block n {n} of {records} +{pre}")
    # above the run's records: refused, nothing written
    a = pose_arena(1, records + 1)
    assert lib().ppf_batch_copy_block(bm.ptr, C.c_void_p(a.ptr), records + 1, None) == _capi.PPF_ERR_INVALID
    torch.cuda.synchronize()
    assert (a.mem.cpu().numpy() == CANARY32).all()
