"""ppf_depth_history on the device against the numpy oracle (tests/depth_history_oracle.py): the fused image and the state
image byte for byte and every count, after every push of a sequence.  Shapes across the kernel's four-pixel lanes and its
workgroup edges, every width 1..130, both formats, pitched inputs whose rows are not 16-byte aligned, the ring's wrap for
several windows, the anchor at every age, min_support, the gate's closures, both modes with a mean whose bytes depend on the
order of the sum, reset, the host and the device entry, the outputs, refused arguments, two threads, a side stream, a window of
the C1 frame through the history and the filter into the normals, ``FuseDepth`` and the C++ demo."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import depth_filter_oracle as F
import depth_history_oracle as H
import depth_normals_oracle as N
import prep_data as D
from test_depth_history_oracle import ORDER_BITS, order_frames, sequence
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import lib
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DepthHistory, DeviceCloud, filter_depth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo_ppf_pose_estimation_amd", "csrc")
DEPTH_KEYS = ("depth_scale", "z_min", "z_max")
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (4, 64), (5, 65), (9, 129), (37, 200)]


def make(shape, dtype=np.float32, **kw):
    """(the device history, the oracle) for the oracle's keywords"""
    dk = {k: v for k, v in kw.items() if k in DEPTH_KEYS}
    prm = {k: v for k, v in kw.items() if k not in DEPTH_KEYS and k != "mean"}
    prm["flags"] = _capi.PPF_HISTORY_MEAN if kw.get("mean") else 0
    return DepthHistory(shape, dtype=dtype, params=prm, **dk), H.History(**kw)


def same(got, want, what):
    got = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint8 if got.dtype == np.uint8 else np.uint32) != want.view(np.uint8 if got.dtype == np.uint8 else np.uint32))
        v, u = bad[0]
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first ({v}, {u}): {got[v, u]!r} against {want[v, u]!r}")


def check_push(dev, ora, frame, feed=None, what=""):
    """one push through both: image, state and counts are the oracle's; returns the oracle's triple"""
    want = ora.push(frame)
    out, state, st = dev.push(frame if feed is None else feed, return_state=True, return_stats=True)
    same(out, want[0], f"{what} out")
    same(state, want[1], f"{what} state")
    assert {k: st[k] for k in H.COUNTS} == want[2], (what, st, want[2])
    assert (st["n_launches"], st["n_host_syncs"]) == (1, 1)
    return want


def check_sequence(frames, **kw):
    dev, ora = make(frames[0].shape, frames[0].dtype, **kw)
    seen = set()
    for t, f in enumerate(frames):
        seen |= set(np.unique(check_push(dev, ora, f, what=f"{frames[0].shape} {kw} push {t}")[1]).tolist())
    assert dev.info()["frames"] == len(frames)
    return seen


def test_shapes_across_lanes_and_workgroups_both_formats():
    rng = np.random.default_rng(41)
    for shape in SHAPES:
        check_sequence(sequence(rng, shape, 8), window=3)
        check_sequence(sequence(rng, shape, 10, dtype=np.uint16), window=4, mean=True, min_support=2)
    seen = check_sequence(sequence(rng, (37, 200), 10), window=8)
    assert seen >= {0, 1, 2, 17}


def test_every_width_up_to_130():
    rng = np.random.default_rng(42)
    for cols in range(1, 131):
        dtype = np.uint16 if cols % 2 else np.float32
        check_sequence(sequence(rng, (3, cols), 5, dtype=dtype), window=3, mean=bool((cols // 2) % 2), min_support=1 + cols % 3)


def test_pitched_device_inputs_whose_rows_are_not_16_byte_aligned():
    import torch
    rng = np.random.default_rng(43)
    for dtype, pad, off, cols in ((np.float32, 3, 1, 64), (np.float32, 5, 2, 61), (np.float32, 4, 0, 64), (np.float32, 8, 4, 60),
                                  (np.uint16, 3, 1, 64), (np.uint16, 6, 2, 63), (np.uint16, 4, 0, 64), (np.uint16, 8, 3, 60)):
        shape = (9, cols)
        frames = sequence(rng, shape, 6, dtype=dtype)
        dev, ora = make(shape, dtype, window=4, mean=dtype == np.uint16)
        for t, f in enumerate(frames):
            wide = np.full((shape[0], cols + pad), 1, dtype)
            wide[:, off:off + cols] = f
            view = torch.from_numpy(wide).cuda()[:, off:off + cols]
            assert not view.is_contiguous() and view.stride(0) == cols + pad
            check_push(dev, ora, f, feed=view, what=f"{dtype.__name__} pad {pad} off {off} push {t}")
            check_push(dev, ora, f, feed=wide[:, off:off + cols], what="host view")      # the host entry reads through the pitch too


@pytest.mark.parametrize("window", [1, 2, 3, 8, 16])
def test_ring_wrap_both_modes_min_support_one_and_window(window):
    rng = np.random.default_rng(44 + window)
    frames = sequence(rng, (13, 37), 2 * window + 2)
    for mean in (False, True):
        seen = check_sequence(frames, window=window, mean=mean, max_age=15)
        check_sequence(frames, window=window, mean=mean, min_support=window, max_age=min(window - 1, 15))
        if window >= 3:
            assert seen >= {0, 1, 2, 17}
    u16 = sequence(rng, (6, 10), 2 * window + 2, dtype=np.uint16)
    check_sequence(u16, window=window, depth_scale=0.000125, range_abs=0.002, range_quad=0.01, z_min=0.12, z_max=0.135)


def test_the_anchor_at_every_age_and_one_past_max_age():
    shape = (5, 9)
    full, hole = np.full(shape, np.float32(1.25)), np.zeros(shape, np.float32)
    for window, max_age in ((16, 5), (8, 7), (4, 15), (16, 15), (3, 0)):        # max_age 15 in a window of 4: larger than n_hist
        dev, ora = make(shape, window=window, max_age=max_age)
        for t in range(min(window, max_age + 1) + 2):
            _, state, counts = check_push(dev, ora, full if t == 0 else hole, what=f"window {window} max_age {max_age} push {t}")
            filled = 1 <= t <= min(max_age, window - 1)
            assert (state == (1 if t == 0 else 2 if filled else 0)).all()
            assert counts["n_filled"] == (state.size if filled else 0)


def test_gate_closures_and_the_order_of_the_mean():
    far = np.float32(1.0078125)
    for older, state in ((far, 1), (np.nextafter(far, np.float32(2)), 17)):
        for mean in (False, True):
            dev, ora = make((1, 2), window=2, range_abs=0.0078125, mean=mean)
            check_push(dev, ora, np.array([[older, older]], np.float32))
            _, st, _ = check_push(dev, ora, np.array([[1.0, 1.0]], np.float32))
            assert (st == state).all()
    dev, ora = make((1, 1), window=4, range_abs=3e38, mean=True)
    for f in order_frames():
        out, _, _ = check_push(dev, ora, f)
    total = 0.0
    for x in ORDER_BITS.view(np.float32):            # newest first: the other order
        total = total + float(x)
    assert out[0, 0].tobytes() != np.float32(total / 4.0).tobytes()


def test_reset_in_mid_sequence_equals_a_fresh_history():
    rng = np.random.default_rng(46)
    frames = sequence(rng, (11, 23), 9)
    dev, ora = make((11, 23), window=4)
    for f in frames[:6]:
        check_push(dev, ora, f)
    dev.reset()
    ora.reset()
    assert dev.info()["frames"] == 0
    fresh, _ = make((11, 23), window=4)
    for f in frames[6:]:
        want = check_push(dev, ora, f)
        out, state, st = fresh.push(f, return_state=True, return_stats=True)
        assert out.tobytes() == want[0].tobytes() and state.tobytes() == want[1].tobytes() and st["frame"] == want[2]["frame"]


def test_host_and_device_entries_outputs_and_refusals():
    import torch
    rng = np.random.default_rng(47)
    shape = (37, 200)
    n = shape[0] * shape[1]
    frames = sequence(rng, shape, 7)
    dev, ora = make(shape, window=4)
    host, _ = make(shape, window=4)
    out_t = torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
    out_h = np.full(shape, np.float32(7.0))
    side = torch.cuda.Stream()
    for t, f in enumerate(frames):
        want = ora.push(f)
        ft = torch.from_numpy(f).cuda()
        if t % 3 == 0:          # out= reuse, no state
            assert dev.push(ft, out=out_t) is out_t and host.push(f, out=out_h) is out_h
            same(out_t, want[0], "device out=")
            same(out_h, want[0], "host out=")
        elif t % 3 == 1:        # a strided tensor on a side stream
            wide = torch.from_numpy(np.ascontiguousarray(np.pad(f, ((0, 0), (8, 16)), constant_values=1.0))).cuda()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                got, state, st = dev.push(wide[:, 8:8 + shape[1]], return_state=True, return_stats=True)
            assert got.is_cuda and state.is_cuda and state.dtype == torch.uint8
            same(got, want[0], "side stream out")
            same(state, want[1], "side stream state")
            assert {k: st[k] for k in H.COUNTS} == want[2]
            same(host.push(f), want[0], "host")
        else:
            got, st = dev.push(ft, return_stats=True)
            same(got, want[0], "device")
            h_out, h_state, h_st = host.push(f, return_state=True, return_stats=True)
            same(h_out, want[0], "host")
            same(h_state, want[1], "host state")
            assert {k: st[k] for k in H.COUNTS} == {k: h_st[k] for k in H.COUNTS} == want[2]
    # refused before anything is launched: the outputs must be what they say and overlap nothing; t stays
    before = dev.info()["frames"]
    buf = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    ft = torch.from_numpy(frames[0]).cuda()
    for call in (lambda: dev.push(buf[:n].view(shape), out=buf[n // 2:n // 2 + n].view(shape)),
                 lambda: dev.push(buf[:n].view(shape), out=buf[:n].view(shape)),
                 lambda: dev.push(ft, out=torch.zeros((shape[0], shape[1] + 1), dtype=torch.float32, device="cuda")),
                 lambda: dev.push(ft, out=torch.zeros(shape, dtype=torch.float32)),
                 lambda: dev.push(ft[:, :-1]), lambda: dev.push(frames[0].astype(np.float64)),
                 lambda: host.push(frames[0], out=np.zeros((shape[0], shape[1] + 1), np.float32))):
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID
    raw = [  # (depth, pitch, out, state): the C entry itself
        (ft.data_ptr(), 0, buf.data_ptr(), buf.data_ptr() + 4 * n - 8),          # state overlaps out
        (ft.data_ptr(), 0, buf.data_ptr(), ft.data_ptr() + 16),                    # state overlaps the image
        (ft.data_ptr(), 4 * shape[1] - 4, buf.data_ptr(), None),                   # pitch below the row
        (ft.data_ptr(), 4 * shape[1] + 2, buf.data_ptr(), None),                   # pitch not a multiple of the element
        (ft.data_ptr() + 2, 0, buf.data_ptr(), None),                              # misaligned image
        (None, 0, buf.data_ptr(), None), (ft.data_ptr(), 0, None, None),           # NULLs
        (out_h.ctypes.data, 0, buf.data_ptr(), None),                              # host memory
    ]
    for depth, pitch, out, state in raw:
        st = _capi.DepthHistoryStats()
        C.memset(C.byref(st), 0x5A, C.sizeof(st))
        s = lib().ppf_depth_history_push_device(dev._ptr, depth, pitch, out, state, None, C.byref(st))
        assert s == _capi.PPF_ERR_INVALID and bytes(st) == bytes(C.sizeof(st)), (depth, pitch, out, state, _capi.last_error())
    img = frames[0]
    for depth, pitch, out in ((img.ctypes.data, 4 * shape[1] - 4, out_h.ctypes.data), (img.ctypes.data, 4 * shape[1] + 2, out_h.ctypes.data),
                              (None, 0, out_h.ctypes.data), (img.ctypes.data, 0, None), (img.ctypes.data + 2, 0, out_h.ctypes.data)):
        st = _capi.DepthHistoryStats()
        C.memset(C.byref(st), 0x5A, C.sizeof(st))
        kept = out_h.copy()
        s = lib().ppf_depth_history_push(host._ptr, depth, pitch, out, None, C.byref(st))
        assert s == _capi.PPF_ERR_INVALID and bytes(st) == bytes(C.sizeof(st)) and out_h.tobytes() == kept.tobytes()
    assert dev.info()["frames"] == before == host.info()["frames"] and float(buf.abs().sum()) == 0.0
    # after all that the next push is still the oracle's, side by side buffers are fine
    want = ora.push(frames[1])
    buf[:n] = torch.from_numpy(frames[1]).cuda().reshape(-1)
    same(dev.push(buf[:n].view(shape), out=buf[n:].view(shape)), want[0], "side by side")
    info = dev.info()
    assert (info["rows"], info["cols"], info["window"]) == (shape[0], shape[1], 4) and info["device_bytes"] >= 4 * 4 * n
    torch.cuda.synchronize()


def test_launches_and_waits_do_not_depend_on_the_content():
    rng = np.random.default_rng(48)
    shape = (37, 200)
    dev, _ = make(shape, window=3)
    stats = [dev.push(img, return_stats=True)[1] for img in (sequence(rng, shape, 1)[0], np.full(shape, np.float32(1.0)), np.zeros(shape, np.float32))]
    assert len({st["n_measured"] for st in stats}) == 3
    assert [(st["n_launches"], st["n_host_syncs"]) for st in stats] == [(1, 1)] * 3
    assert [st["frame"] for st in stats] == [0, 1, 2]


def test_two_histories_pushed_from_two_threads():
    rng = np.random.default_rng(49)
    seqs = [sequence(rng, (60, 300), 6), sequence(rng, (60, 300), 6, dtype=np.uint16)]
    kws = [dict(window=4), dict(window=3, mean=True)]
    want = []
    for frames, kw in zip(seqs, kws):
        ora = H.History(**kw)
        want.append([tuple(x.tobytes() for x in ora.push(f)[:2]) for f in frames])
    pairs = [make((60, 300), seqs[j][0].dtype, **kws[j]) for j in range(2)]
    got = [None, None]

    def work(j):
        got[j] = [tuple(x.tobytes() for x in pairs[j][0].push(f, return_state=True)) for f in seqs[j]]
    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got == want


def test_c1_window_through_the_history_and_the_filter_into_the_normals():
    import torch
    _, depth, box, intr = D.c1_frame()
    x, y, w, h = box
    r0 = int(np.clip(y + h // 2 - 80, 0, depth.shape[0] - 160))
    c0 = int(np.clip(x + w // 2 - 112, 0, depth.shape[1] - 224))
    win = np.ascontiguousarray(depth[r0:r0 + 160, c0:c0 + 224])
    shifted = (intr[0], intr[1], intr[2] - c0, intr[3] - r0)
    rng = np.random.default_rng(50)
    kw = dict(window=4, range_abs=0.004, range_quad=0.004, mean=True)
    dev, ora = make(win.shape, **kw)
    cp = CloudProcessor(None, None, [], [], [], 0.05, 0.05)
    for t in range(5):
        frame = np.where(rng.random(win.shape) < 0.1, np.float32(0), win + (0.001 * rng.standard_normal(win.shape)).astype(np.float32) * win * win)
        frame = np.ascontiguousarray(frame, np.float32)
        want_img, want_state, counts = ora.push(frame)
        fused = dev.push(torch.from_numpy(frame).cuda())
        assert fused.is_cuda
        same(fused, want_img, f"push {t}")
        got = cp.FuseDepth(frame, params=dict(window=4, range_abs=0.004, range_quad=0.004, flags=_capi.PPF_HISTORY_MEAN))
        assert got is cp.depth and got.tobytes() == want_img.tobytes() and cp.depth_state.tobytes() == want_state.tobytes()
        assert {k: cp.depth_history_stats[k] for k in H.COUNTS} == counts
    assert counts["n_filled"] > 1000 and counts["n_measured"] > 5000
    want_filtered, fcounts = F.filter_depth(want_img)
    want_rows, want_curv = N.depth_normals(want_filtered, shifted, fp64=True)
    filtered = filter_depth(fused)
    rows, curv = DeviceCloud.from_depth(filtered, shifted, fp64=True, normals={}).download()
    assert filtered.is_cuda and rows.tobytes() == want_rows.tobytes() and curv.tobytes() == want_curv.tobytes()
    assert cp.FilterDepth().tobytes() == want_filtered.tobytes() and cp.depth_filter_stats["n_unsupported"] == fcounts["n_unsupported"]
    # other parameters, or another shape: the processor starts a new history
    cp.FuseDepth(frame)
    assert cp.depth_history_stats["frame"] == 0
    cp.FuseDepth(frame)
    cp.FuseDepth(frame[:, :-1])
    assert cp.depth_history_stats["frame"] == 0 and cp.depth.shape == (160, 223)


def words(a):
    return int(np.ascontiguousarray(a).view(np.uint32).astype(np.uint64).sum())


def demo_noisy(depth, frame, noise, seed):
    """examples/depth_history_demo.cpp's stream"""
    n = depth.size
    x = np.uint64(seed) + np.uint64(frame) * np.uint64(n) + np.arange(n, dtype=np.uint64)
    h = x * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(32)
    h *= np.uint64(0xD6E8FEB86659FD93)
    h ^= h >> np.uint64(32)
    dropped = ((h >> np.uint64(16)) & np.uint64(255)) < 26
    z = (depth.ravel().astype(np.float64) + noise * ((h & np.uint64(65535)).astype(np.float64) / 65536.0 - 0.5)).astype(np.float32)
    return np.where(dropped, np.float32(0), z).reshape(depth.shape)


def test_cpp_demo_matches_the_python_route(tmp_path, bottle):
    from test_gpu_frame import _render_frame
    _, depth, _, K, _, _ = _render_frame(bottle)
    depth = np.ascontiguousarray(depth, np.float32)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    exe = str(tmp_path / "depth_history_demo")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "depth_history_demo.cpp"), "-L", CSRC, "-lppf_hip", f"-Wl,-rpath,{CSRC}", "-o", exe], check=True)
    (tmp_path / "depth.f32").write_bytes(depth.tobytes())
    for frames, prm, noise, seed in ((6, dict(window=4, range_abs=0.01, range_quad=0.0, min_support=1, max_age=7, flags=0), 0.004, 1),
                                     (5, dict(window=3, range_abs=0.003, range_quad=0.002, min_support=2, max_age=1, flags=1), 0.006, 12345)):
        args = [str(frames), str(prm["window"]), repr(float(prm["range_abs"])), repr(float(prm["range_quad"])), str(prm["min_support"]),
                str(prm["max_age"]), str(prm["flags"]), repr(noise), str(seed)]
        r = subprocess.run([exe, str(tmp_path / "depth.f32"), str(depth.shape[0]), str(depth.shape[1])] + [repr(float(v)) for v in intr] + args,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        hist = DepthHistory(depth.shape, params=prm)
        want = []
        for k in range(frames):
            fused, state, st = hist.push(demo_noisy(depth, k, noise, seed), return_state=True, return_stats=True)
            want.append(f"frame {st['frame']} kept {st['n_kept']} measured {st['n_measured']} filled {st['n_filled']} "
                        f"unsupported {st['n_unsupported']} empty {st['n_empty']} changed {st['n_changed']}")
        want.append(f"history {depth.shape[0]} x {depth.shape[1]} window {prm['window']} frames {frames}")
        want.append(f"fused image checksum {words(fused)} state checksum {int(state.astype(np.uint64).sum())}")
        filtered, fs = filter_depth(fused, return_stats=True)
        want.append(f"filtered kept {fs['n_kept']} unsupported {fs['n_unsupported']} written {fs['n_written']} checksum {words(filtered)}")
        rows, curv = DeviceCloud.from_depth(filtered, intr, fp64=True, normals={}).download()
        want.append(f"cloud rows {rows.shape[0]} checksum {words(rows) + words(curv)}")
        assert r.stdout.strip().splitlines() == want
        assert st["n_filled"] > 0 and st["n_measured"] > 0
