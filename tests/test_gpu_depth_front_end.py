"""The host front end the depth-image stages share (csrc/ppf_depthimage_host.h), on the device: one 5 x 67
image -- 67 crosses the 64-column tiles of the filter and the segments and is no multiple of 4, so the history's vector
paths are off; 5 rows cross the 4-row tiles -- goes through all five stages (cloud, with and without normals; register;
filter; history; segments) in both formats, by the host entries as a packed array and as a row-strided view with an odd pitch,
and by the device entries as a row-strided GPU tensor on a side stream with ``out=``.  Everything the three ways give is
byte-equal: clouds, images, labels, state, records and counters.  An ``out`` that overlaps the input is PPF_ERR_INVALID before
any launch, for every stage that has one; and behind a real map and a real history, register and push check in the order
they always had."""
import numpy as np
import pytest
import torch

from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.cloud_processor import DepthHistory, DepthMap, DeviceCloud, filter_depth, segment_depth

pytestmark = pytest.mark.gpu

ROWS, COLS, WIDE, LEFT = 5, 67, 71, 2          # the views: columns LEFT .. LEFT + COLS of rows of WIDE elements
INTR = (60.0, 61.0, 33.0, 2.5)
COLOR_SHAPE = (6, 70)
DEPTH = dict(depth_scale=0.001, z_min=0.2, z_max=3.0)
FORMATS = [np.float32, np.uint16]


def frames(dtype):
    """two frames of a tilted plane with a step at column 40, holes, and a few pixels outside the z range"""
    v, u = np.mgrid[0:ROWS, 0:COLS]
    z = 1.0 + 0.002 * u + 0.003 * v + np.where(u >= 40, 0.3, 0.0)
    rng = np.random.default_rng(67)
    out = []
    for t in range(2):
        f = z + 0.0005 * t + rng.normal(0.0, 0.0003, z.shape)
        f[rng.random(z.shape) < 0.08] = 0.0
        f[1 + t, 5], f[3, 66 - t] = 5.0, 0.1
        out.append(np.round(f * 1000.0).astype(np.uint16) if dtype == np.uint16 else f.astype(np.float32))
    if dtype == np.float32:
        out[0][0, 64], out[1][4, 0] = np.nan, np.inf
    return out


def strided(f):
    wide = np.full((ROWS, WIDE), 1, f.dtype)
    wide[:, LEFT:LEFT + COLS] = f
    return wide[:, LEFT:LEFT + COLS]


def make_map():
    return DepthMap(INTR, (ROWS, COLS), (62.0, 62.5, 35.0, 3.0), COLOR_SHAPE, np.eye(3), (0.01, -0.002, 0.001))


def counters(st):
    return {k: v for k, v in st.items() if k != "ms_wall"}


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def run_stages(fs, device):
    """every stage's results as a flat list of arrays and dicts; device: GPU tensors on a side stream, out= supplied"""
    res = []
    dmap, hist = make_map(), DepthHistory((ROWS, COLS), dtype=fs[0].dtype, params=dict(window=3, min_support=1), **DEPTH)
    side = torch.cuda.Stream() if device else None

    def outs(shape, dtype):
        return dict(out=torch.full(shape, 7, dtype=dtype, device="cuda")) if device else {}

    def stages(f):
        for normals in (None, dict(radius=2)):
            res.extend(DeviceCloud.from_depth(f, INTR, normals=normals, **DEPTH).download())
        img, st = dmap.register(f, return_stats=True, **DEPTH, **outs(COLOR_SHAPE, torch.float32))
        res.extend([host(img), counters(st)])
        img, st = filter_depth(f, params=dict(radius=2, min_support=3), return_stats=True, **DEPTH, **outs((ROWS, COLS), torch.float32))
        res.extend([host(img), counters(st)])
        lab, info, counts, st = segment_depth(f, params=dict(min_size=4), return_info=True, return_stats=True, **DEPTH,
                                              **outs((ROWS, COLS), torch.int32))
        res.extend([host(lab), info, counts, counters(st)])
        img, state, st = hist.push(f, return_state=True, return_stats=True, **outs((ROWS, COLS), torch.float32))
        res.extend([host(img), host(state), counters(st)])

    for f in fs:
        if device:
            t = torch.from_numpy(np.ascontiguousarray(f.base)).cuda()[:, LEFT:LEFT + COLS]
            assert t.stride(0) == WIDE and not t.is_contiguous()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                stages(t)
        else:
            stages(f)
    return res


@pytest.mark.parametrize("dtype", FORMATS, ids=["f32", "u16"])
def test_host_and_device_entries_agree_byte_for_byte(dtype):
    fs = frames(dtype)
    views = [strided(f) for f in fs]
    assert all(v.strides == (WIDE * v.itemsize, v.itemsize) and not v.flags.c_contiguous for v in views)
    packed, pitched, device = run_stages(fs, False), run_stages(views, False), run_stages(views, True)
    assert len(packed) == len(pitched) == len(device) == 2 * 15
    for k, (a, b, c) in enumerate(zip(packed, pitched, device)):
        if isinstance(a, dict):
            assert a == b == c, (k, a, b, c)
        else:
            assert a.dtype == b.dtype == c.dtype and a.shape == b.shape == c.shape, k
            assert a.tobytes() == b.tobytes() == c.tobytes(), k
    # the image was worth the trouble: points on both sides of the step, a filled register image, two segments, filled holes
    assert len(packed[0]) > 200 and packed[5]["n_filled"] > 0 and packed[7]["n_kept"] > 200 and packed[10][0] >= 2
    assert packed[15 + 14]["n_filled"] > 0 and packed[15 + 14]["frame"] == 1


@pytest.mark.parametrize("dtype", FORMATS, ids=["f32", "u16"])
def test_an_out_that_overlaps_the_input_is_refused_before_any_launch(dtype):
    f = frames(dtype)[0]
    raw = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    depth = raw[:f.nbytes].view(torch.float32 if dtype == np.float32 else torch.uint16).view(ROWS, COLS)
    depth.copy_(torch.from_numpy(f).cuda())
    before = depth.clone()

    def over(shape, tdtype, at):
        """a contiguous out that starts `at` bytes into the input"""
        n = shape[0] * shape[1] * 4
        return raw[at:at + n].view(tdtype).view(shape)

    dmap, hist = make_map(), DepthHistory((ROWS, COLS), dtype=dtype, **DEPTH)
    calls = [
        ("ppf_depth_filter_device", lambda: filter_depth(depth, out=over((ROWS, COLS), torch.float32, 8), **DEPTH)),
        ("ppf_depth_filter_device", lambda: filter_depth(depth, out=over((ROWS, COLS), torch.float32, (f.nbytes - 4) // 4 * 4), **DEPTH)),
        ("ppf_depth_register_device", lambda: dmap.register(depth, out=over(COLOR_SHAPE, torch.float32, 16), **DEPTH)),
        ("ppf_depth_segments_device", lambda: segment_depth(depth, out=over((ROWS, COLS), torch.int32, 4), **DEPTH)),
        ("ppf_depth_history_push_device", lambda: hist.push(depth, out=over((ROWS, COLS), torch.float32, 12))),
    ]
    for entry, call in calls:
        with pytest.raises(_capi.PPFError) as e:
            call()
        assert e.value.status == _capi.PPF_ERR_INVALID, entry
        what = "label buffer" if "segments" in entry else "output"
        assert str(e.value).endswith(f"{entry}: the {what} overlaps the image"), str(e.value)
    torch.cuda.synchronize()
    assert torch.equal(depth.view(torch.uint8), before.view(torch.uint8)) and hist.info()["frames"] == 0   # nothing ran
    # an out right behind the input is fine
    got = filter_depth(depth, out=over((ROWS, COLS), torch.float32, (f.nbytes + 15) // 16 * 16), **DEPTH)
    assert got.cpu().numpy().tobytes() == filter_depth(f, **DEPTH).tobytes()


def test_register_and_push_keep_their_check_order_behind_a_real_handle():
    """what tests/test_depth_entry_errors.py cannot reach without a device: the checks behind the map and the history, and
    which of two errors wins (the texts are those of the entries before they shared the front end)"""
    import ctypes as C
    lib = _capi.lib()
    dmap, hist = make_map(), DepthHistory((ROWS, COLS), **DEPTH)
    img = frames(np.float32)[0]
    dev = torch.from_numpy(img).cuda()
    out_h, out_d = np.full(COLOR_SHAPE, np.float32(7.0)), torch.full(COLOR_SHAPE, 7.0, device="cuda")

    def register(device, pitch=0, **kw):
        dp, rp, st = _capi.DepthParams(), _capi.RegisterParams(), _capi.RegisterStats()
        lib.ppf_default_depth_params(C.byref(dp))
        lib.ppf_default_register_params(C.byref(rp))
        for k, v in kw.items():
            setattr(rp if k.startswith("quad") or k == "rflags" else dp, "flags" if k == "rflags" else k, v)
        st.n_launches = 7
        if device:
            s = lib.ppf_depth_register_device(dmap._ptr, C.c_void_p(dev.data_ptr()), pitch, C.byref(dp), C.byref(rp), C.c_void_p(out_d.data_ptr()),
                                              None, C.byref(st))
        else:
            s = lib.ppf_depth_register(dmap._ptr, C.c_void_p(img.ctypes.data), pitch, C.byref(dp), C.byref(rp), C.c_void_p(out_h.ctypes.data),
                                       C.byref(st))
        return s, _capi.last_error(), st.n_launches

    width = COLS * 4
    cases = [
        (dict(flags=1, z_max=-1.0), "the depth params' flags must be 0 here (0x1)"),
        (dict(flags=1, pitch=20), "the depth params' flags must be 0 here (0x1)"),
        (dict(format=2, rflags=1), "unknown depth format 2"),
        (dict(pitch=20, z_max=-1.0), f"row pitch 20 bytes is below {width} or not a multiple of 4"),
        (dict(z_max=-1.0, rflags=1), "z_min and z_max must be finite and z_max >= 0"),
        (dict(quad_dz_abs=-1.0, rflags=1), "quad_dz_abs and quad_dz_rel must be finite and >= 0"),
        (dict(rflags=1), "unknown flags 0x1"),
    ]
    for device in (False, True):
        entry = "ppf_depth_register_device" if device else "ppf_depth_register"
        for kw, text in cases:
            out_h[:] = 7.0
            s, err, launches = register(device, **kw)
            assert s == _capi.PPF_ERR_INVALID and err == f"{entry}: {text}" and launches == 0, (entry, kw, err)
            assert device or not out_h.any()                   # the host entry alone leaves a failed call's out zero
    torch.cuda.synchronize()
    assert (out_d == 7.0).all()

    st = _capi.DepthHistoryStats()
    res = np.full((ROWS, COLS), np.float32(7.0))
    for device in (False, True):
        st.n_launches = 7
        if device:
            s = lib.ppf_depth_history_push_device(hist._ptr, C.c_void_p(dev.data_ptr()), 20, C.c_void_p(out_d.data_ptr()), None, None, C.byref(st))
        else:
            s = lib.ppf_depth_history_push(hist._ptr, C.c_void_p(img.ctypes.data), 20, C.c_void_p(res.ctypes.data), None, C.byref(st))
        entry = "ppf_depth_history_push" + ("_device" if device else "")
        assert s == _capi.PPF_ERR_INVALID and st.n_launches == 0
        assert _capi.last_error() == f"{entry}: row pitch 20 bytes is below {width} or not a multiple of 4"
    assert (res == 7.0).all() and hist.info()["frames"] == 0
