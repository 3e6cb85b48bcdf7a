"""ppf_select_frame's C-ABI surface without a GPU: the three structs as a C compiler lays them out equal their ctypes
mirrors, the defaults, every argument error comes before any device work (zeroed info rows, selected all -1, n_selected 0,
images all 0 and all -1), and a valid call fails loudly (PPF_ERR_HIP) when there is no device.  Also the figures of
DESIGN.md §16 from the numpy oracle (tests/select_oracle.py) on the oracle poses of tests/golden/select_two_bottles.npz:
which hypotheses explain the depth image, and that the greedy selection keeps exactly one pose per bottle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import render_oracle as R
import select_oracle as S
from test_gpu_frame import _render_frame
from test_verify_capi import INTR, _dets
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import Pose, PoseScore, RenderParams, SelectInfo, SelectParams, SelectStats, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAN, INF = float("nan"), float("inf")
TOP = 8


def test_select_struct_layouts_match_the_header(tmp_path):
    structs = [("ppf_select_params", SelectParams), ("ppf_select_info", SelectInfo), ("ppf_select_stats", SelectStats)]
    expr, got = [], []
    for cname, cls in structs:
        expr.append(f"sizeof({cname})")
        got.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            expr.append(f"offsetof({cname}, {f})")
            got.append(getattr(cls, f).offset)
    expr += ["PPF_SELECT_NONE", "PPF_SELECT_SELECTED", "PPF_SELECT_GATED", "PPF_SELECT_SUPPRESSED", "PPF_ABI_VERSION"]
    got += [_capi.PPF_SELECT_NONE, _capi.PPF_SELECT_SELECTED, _capi.PPF_SELECT_GATED, _capi.PPF_SELECT_SUPPRESSED, 4]
    src = tmp_path / "ssz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppf_hip.h"\nint main(void){\n' +
                   "".join(f'printf("%zu\\n", (size_t)({e}));\n' for e in expr) + "return 0;}\n")
    exe = tmp_path / "ssz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert (S.NONE, S.SELECTED, S.GATED, S.SUPPRESSED) == (0, 1, 2, 3)
    assert S.INFO.itemsize == C.sizeof(SelectInfo) and [S.INFO.fields[f][1] for f, _ in SelectInfo._fields_] == \
        [getattr(SelectInfo, f).offset for f, _ in SelectInfo._fields_]


def test_symbols_are_exported_and_bound():
    L = C.CDLL(_capi.LIB_PATH)
    for name in ("ppf_default_select_params", "ppf_select_frame"):
        assert hasattr(L, name) and name in _capi._SIGNATURES
    assert lib().ppf_abi_version() == 4


def sdefaults():
    p = SelectParams()
    p.depth_tol, p.max_overlap, p.min_score, p.min_pixels, p.flags = 7.0, 7.0, 7.0, 7, 7
    for i in range(4):
        p.reserved[i] = 7
    lib().ppf_default_select_params(C.byref(p))
    return p


def rdefaults():
    p = RenderParams()
    lib().ppf_default_render_params(C.byref(p))
    return p


def test_select_defaults():
    p = sdefaults()
    assert (p.depth_tol, p.max_overlap, p.min_score, p.min_pixels, p.flags) == (C.c_float(0.01).value, 0.25, 0.0, 1, 0)
    assert list(p.reserved) == [0, 0, 0, 0]
    assert S.DEFAULTS == dict(depth_tol=0.01, max_overlap=0.25, min_score=0.0, min_pixels=1)
    lib().ppf_default_select_params(None)   # no crash


def _call(dets, n_dets, n_poses=None, top=4, rows=6, cols=5, intr=INTR, p=None, rp=None, poses=True, counts=True, depth=True, scores=False,
          infos=True, sel=True, nsel=True, params=True, rparams=True, images=True):
    np_ = (C.c_int * 300)(*([2] * 300 if n_poses is None else n_poses))
    ps = (Pose * (300 * 16))() if poses else None
    sc = (PoseScore * (300 * 16))() if scores else None
    info = (SelectInfo * (300 * 16))()
    for i in range(len(info)):
        info[i].status, info[i].key = 77, 7.0   # garbage the call must clear
    chosen = (C.c_int * (300 * 16))(*([55] * (300 * 16)))
    n_sel = C.c_int(66)
    it = (C.c_double * 4)(*intr) if intr is not None else None
    n = max(rows * cols, 1) if 0 < rows < 100 and 0 < cols < 100 else 1
    img = np.ones(n, dtype=np.float32)
    out_d = np.full(n + 1, 9.0, dtype=np.float32)
    out_l = np.full(n + 1, 9, dtype=np.int32)
    prm = sdefaults() if p is None else p
    rprm = rdefaults() if rp is None else rp
    st = SelectStats()
    st.n_launches = 99
    s = lib().ppf_select_frame(dets, n_dets, ps, np_ if counts else None, top, sc, img.ctypes.data if depth else None, rows, cols, it,
                               C.byref(rprm) if rparams else None, C.byref(prm) if params else None, info if infos else None,
                               chosen if sel else None, C.byref(n_sel) if nsel else None, out_d.ctypes.data if images else None,
                               out_l.ctypes.data if images else None, C.byref(st))
    return s, info, chosen, n_sel, out_d, out_l, st


def _cleared(r, n_dets, top=4, sized=True):
    s, info, chosen, n_sel, out_d, out_l, st = r
    ok = n_sel.value == 0
    if 0 < n_dets <= 256 and 1 <= top <= 16:
        n = n_dets * top
        ok = ok and all(bytes(info[i]) == bytes(SelectInfo()) for i in range(n)) and list(chosen[:n]) == [-1] * n
        ok = ok and info[n].status == 77 and chosen[n] == 55   # nothing beyond them is touched
    if sized:
        ok = ok and (out_d[:-1] == 0).all() and (out_l[:-1] == -1).all() and out_d[-1] == 9.0 and out_l[-1] == 9
    return bool(ok)


def _invalid(r, n_dets=3, top=4, needle=None, sized=True):
    s, st = r[0], r[-1]
    assert s == _capi.PPF_ERR_INVALID, (s, _capi.last_error())
    assert "ppf_select_frame" in _capi.last_error()
    if needle:
        assert needle in _capi.last_error(), _capi.last_error()
    assert st.n_launches == 0 and st.n_host_syncs == 0 and st.n_jobs == 0 and st.n_selected == 0
    assert _cleared(r, n_dets, top, sized)


def test_select_range_and_null_errors():
    dets = _dets(3)
    _invalid(_call(dets, 257), n_dets=257, needle="n_dets")
    _invalid(_call(dets, -1), n_dets=-1, needle="n_dets")
    for top in (0, 17):
        _invalid(_call(dets, 3, top=top), top=top, needle="top")
    _invalid(_call(dets, 3, n_poses=[2, 5, 1]), needle="n_poses[1]")
    _invalid(_call(dets, 3, n_poses=[2, -1, 1]), needle="n_poses[1]")
    _invalid(_call(dets, 3, params=False), needle="params")
    _invalid(_call(dets, 3, rparams=False), needle="rparams")
    _invalid(_call(dets, 3, poses=False))
    _invalid(_call(dets, 3, counts=False))
    _invalid(_call(None, 3))
    _invalid(_call(dets, 3, depth=False), needle="depth")
    _invalid(_call(_dets(3, model_cloud=False), 3), needle="detection 0")
    s, *_ = _call(dets, 3, infos=False)
    assert s == _capi.PPF_ERR_INVALID
    s, *_ = _call(dets, 3, sel=False)
    assert s == _capi.PPF_ERR_INVALID
    s, *_ = _call(dets, 3, nsel=False)
    assert s == _capi.PPF_ERR_INVALID and "n_selected" in _capi.last_error()
    r = _call(dets, 3, intr=None, images=False, scores=True)   # NULL images are allowed, the error still comes
    assert r[0] == _capi.PPF_ERR_INVALID and _cleared(r, 3, sized=False)
    # a detection without a model cloud and without poses is skipped, not an error: the call gets as far as the device
    if lib().ppf_device_count() == 0:
        assert _call(_dets(3, model_cloud=False), 3, n_poses=[0, 0, 0])[0] == _capi.PPF_ERR_HIP


def test_select_parameter_errors():
    dets = _dets(3)
    for field, values in (("depth_tol", (0.0, -0.01, NAN, INF)), ("max_overlap", (-0.01, 1.01, NAN, INF)), ("min_score", (NAN, INF, -INF)),
                          ("min_pixels", (0, -3)), ("flags", (1, -1, 4))):
        for v in values:
            p = sdefaults()
            setattr(p, field, v)
            _invalid(_call(dets, 3, p=p), needle=field)
    for field, values in (("splat_radius", (0.0, -0.001, NAN, INF)), ("visible_tol", (0.0, -1.0, NAN, INF)), ("flags", (1, -1, 4))):
        for v in values:
            rp = rdefaults()
            setattr(rp, field, v)
            _invalid(_call(dets, 3, rp=rp), needle=field)


def test_select_image_errors():
    dets = _dets(3)
    for rows, cols in ((0, 5), (6, 0), (-1, 5), (70000, 70000)):
        _invalid(_call(dets, 3, rows=rows, cols=cols), sized=False)
    _invalid(_call(dets, 3, intr=None), needle="intr")
    for bad in ((0.0, 1.0, 2.0, 2.0), (1.0, -1.0, 2.0, 2.0), (-5.0, 1.0, 2.0, 2.0), (NAN, 1.0, 2.0, 2.0), (1.0, INF, 2.0, 2.0),
                (1.0, 1.0, NAN, 2.0), (1.0, 1.0, 2.0, -INF)):
        _invalid(_call(dets, 3, intr=bad))


def test_select_without_a_device_is_loud():
    if lib().ppf_device_count() > 0:
        pytest.skip("a GPU is present")
    for n, kw in ((0, {}), (3, {}), (3, dict(scores=True)), (3, dict(n_poses=[0, 0, 0])), (3, dict(images=False))):
        r = _call(_dets(n), n, **kw)
        assert r[0] == _capi.PPF_ERR_HIP, _capi.last_error()
        assert "no HIP device" in _capi.last_error() and "ppf_select_frame" in _capi.last_error()
        assert r[-1].n_launches == 0 and r[-1].n_host_syncs == 0
        assert _cleared(r, n, sized=kw.get("images", True))


# ---- the figures of DESIGN.md §16: the numpy oracle on the oracle poses of the two-bottle frame ------------------------------
@pytest.fixture(scope="module")
def two_bottles(bottle):
    fx = np.load(os.path.join(GOLDEN, "select_two_bottles.npz"))
    _, depth, boxes, K, objs, _ = _render_frame(bottle)
    intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    assert fx["boxes"].tolist() == [list(boxes[0]), list(boxes[1]), [72, 142, 309, 83]]
    assert fx["n_poses"].tolist() == [TOP] * 3
    assert np.array_equal(fx["true_poses"], np.array([objs[0][1], objs[1][1]]))
    hyps = [(i * TOP + k, R.move_np(bottle, fx["poses"][i, k])) for i in range(3) for k in range(TOP)]
    return dict(hyps=hyps, depth=depth, intr=intr, poses=fx["poses"], true=fx["true_poses"])


def _select(tb, **kw):
    return S.select(tb["hyps"], 3 * TOP, tb["depth"], tb["intr"], 0.003, **dict(S.DEFAULTS, **kw))


def test_oracle_explained_shares(two_bottles):
    info = _select(two_bottles)["info"].reshape(3, TOP)
    assert info[0, 0]["explained"] >= 0.79 and info[1, 0]["explained"] >= 0.79
    assert info[2, 0]["explained"] <= 0.18 and info[2, 4]["explained"] <= 0.18
    for i, k in ((0, 0), (1, 0)):   # explained is the fp32 of the fp64 quotient of the two counts
        r = info[i, k]
        assert r["explained"] == np.float32(float(r["n_supported"]) / float(r["n_drawn"])) and 0 < r["n_supported"] <= r["n_drawn"]


@pytest.mark.parametrize("max_overlap", [0.1, 0.25, 0.5])
def test_oracle_selection_with_the_gate(two_bottles, max_overlap):
    got = _select(two_bottles, min_score=0.3, max_overlap=max_overlap)
    assert got["n_selected"] == 2 and got["selected"][:2].tolist() == [0 * TOP + 0, 1 * TOP + 0]
    assert (got["selected"][2:] == -1).all()
    info = got["info"].reshape(3, TOP)
    assert info[0, 0]["rank"] == 0 and info[1, 0]["rank"] == 1
    # one selected pose per bottle, each at its bottle (the oracles give 1.5 mm)
    model = np.load(os.path.join(GOLDEN, "bottle_model_xyzn.npy"))[:, :3].astype(np.float64)
    for b, (i, k) in enumerate(((0, 0), (1, 0))):
        P, T = two_bottles["poses"][i, k], two_bottles["true"][b]
        dist = np.linalg.norm((model @ P[:3, :3].T + P[:3, 3]) - (model @ T[:3, :3].T + T[:3, 3]), axis=1).mean()
        assert dist <= 0.003, (b, dist)
    assert set(np.unique(got["label"])) == {-1, 0, TOP}


def test_oracle_selection_without_the_gate(two_bottles):
    got = _select(two_bottles, min_score=0.0, max_overlap=0.25)
    assert got["selected"][:got["n_selected"]].tolist() == [0 * TOP + 0, 1 * TOP + 0, 2 * TOP + 4, 0 * TOP + 1]
    info = got["info"].reshape(3, TOP)
    # (0, 3) has the counts of (0, 0): the tie goes to the lower j, and the other is suppressed by it
    assert info[0, 3]["n_drawn"] == info[0, 0]["n_drawn"] and info[0, 3]["n_supported"] == info[0, 0]["n_supported"]
    assert info[0, 3]["status"] == S.SUPPRESSED and info[0, 3]["suppressed_by"] == 0
    assert info[0, 3]["n_overlap"] >= 0.9 * info[0, 3]["n_supported"]
    assert info[2, 1]["status"] == S.SUPPRESSED and info[2, 1]["suppressed_by"] == 0   # the same pose through the union box
    assert info[1, 2]["status"] == S.SUPPRESSED and info[1, 2]["suppressed_by"] == TOP
