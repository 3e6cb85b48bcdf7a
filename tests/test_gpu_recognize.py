"""ppf_recognizer_* and ppf_recognize_frame on the device against the numpy oracle (tests/recognize_oracle.py): everything is
compared for equality -- the sorted key tuples, the integers and the fp64 scores bit for bit.  Key sets of four small models
(one with 72 angle bins, whose set is read from global memory), proposals of 0 .. 513 rows with non-finite rows, coincident
points, exactly parallel normals and a NULL cloud, one call against the calls made one by one, repeated calls, a recogniser
of eight 12-degree models next to one of mixed bins and sampling steps, the gates and the tie rule, the refused Darboux
model, the launch and wait counts, recognition models of untouched rows naming all four solids, and CloudProcessor.RecognizeFrame."""
import numpy as np
import pytest

import recognize_cases as K
import recognize_oracle as R
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd.cloud_processor import CloudProcessor, DeviceCloud, Recognizer
from yolo_ppf_pose_estimation_amd.detector import PPF3DDetector

pytestmark = pytest.mark.gpu

INT32_MIN = -(2 ** 31)
# kind, numAngles, presampled rows
MODELS = [("box", 30, 300), ("cylinder", 30, 250), ("torus", 72, 200), ("bottle", 30, 400)]


def turned_box() -> np.ndarray:
    """synth's box turned about z by the angle whose cosine and sine are 0.6 and 0.8: as float32 its side normals have a dot
    product with themselves above 1, so pairs on one face have a NaN angle and the bin INT32_MIN"""
    b = K.solid("box").astype(np.float64)
    Rz = np.array([[0.6, -0.8, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]])
    c = b[:, :3].mean(axis=0)
    return np.concatenate([(b[:, :3] - c) @ Rz.T + c, b[:, 3:6] @ Rz.T], axis=1).astype(np.float32)


def full_cloud(kind: str) -> np.ndarray:
    return turned_box() if kind == "box" else K.solid(kind)


def train(kind: str, num_angles: float, rows: int, step: float = 0.05, seed: int = 1, **kw) -> PPF3DDetector:
    return PPF3DDetector(step, 0.05, num_angles, **kw).trainModel(K.thin(full_cloud(kind), rows, seed), presampled=True)


@pytest.fixture(scope="module")
def dets():
    return [train(*m) for m in MODELS]


@pytest.fixture(scope="module")
def rec(dets):
    return Recognizer(dets)


@pytest.fixture(scope="module")
def oracle_models(dets):
    return [R.Model.from_detector(d) for d in dets]


@pytest.fixture(scope="module")
def proposals():
    """(name, cloud or None): the row counts around the 64-row slice of a scoring workgroup and past max_rows, and the odd clouds"""
    views = {k: K.one_sided_view(full_cloud(k), 40 + i) for i, k in enumerate(K.KINDS)}
    out = [("empty", np.zeros((0, 6), np.float32)), ("null", None)]
    for n, kind in ((1, "box"), (2, "cylinder"), (63, "torus"), (64, "bottle"), (65, "box"), (513, "cylinder"), (300, "torus"), (260, "bottle")):
        out.append((f"{kind}{n}", K.thin(views[kind], n, seed=n)))
    bad = K.thin(views["bottle"], 130, seed=3)
    bad[5, 0] = np.nan
    bad[17, 4] = np.inf
    bad[64, 2] = -np.inf
    bad[129, 5] = np.nan
    out.append(("nonfinite", bad))
    twin = K.thin(views["cylinder"], 90, seed=4)
    twin[10:20] = twin[30:40]  # coincident points with equal normals
    twin[50, :3] = twin[51, :3]  # coincident points with different normals
    out.append(("coincident", twin))
    face = turned_box()
    face = face[np.abs(face[:, 3] - np.float32(0.6)) < 1e-6]  # one side face: every normal (0.6, 0.8, 0) as float32
    out.append(("parallel", K.thin(face, 100, seed=5)))
    return out


def same_scores(got, want, top, where):
    """a proposal's ranked rows against the oracle's: the model order and every field, the doubles by their bytes"""
    assert [int(r["model"]) for r in got] == want["ranked"][:top], (where, got, want["ranked"], want["scores"])
    for r in got:
        m = int(r["model"])
        assert (int(r["n_known"]), int(r["n_keys_hit"])) == tuple(int(v) for v in want["counts"][m]), where
        mine = np.array([r["precision"], r["recall"], r["score"]], dtype=np.float64)
        assert mine.tobytes() == want["scores"][m].tobytes(), (where, m, mine, want["scores"][m])


def check_call(rec, oracle_models, clouds, **prm):
    """one call over `clouds` (arrays or None) equals the oracle; returns what the device gave"""
    dev = [None if c is None else DeviceCloud.upload(c) for c in clouds]
    ranked, n_used, counts, st = rec.recognize(dev, prm, return_counts=True, return_stats=True)
    top = prm.get("top", 2)
    want = R.recognize(clouds, oracle_models, max_rows=prm.get("max_rows", 512), top=top, min_score=prm.get("min_score", 0.0),
                       min_precision=prm.get("min_precision", 0.0))
    for i, w in enumerate(want):
        assert int(n_used[i]) == w["n_used"], (i, n_used[i], w["n_used"])
        assert np.array_equal(counts[i], w["counts"]), (i, counts[i], w["counts"])
        same_scores(ranked[i], w, top, i)
    assert st["n_host_syncs"] == 1 and st["n_clouds"] == len(clouds) and st["n_models"] == len(oracle_models)
    return ranked, n_used, counts, st


def test_key_sets_equal_the_oracle(rec, dets, oracle_models):
    for i, (det, om) in enumerate(zip(dets, oracle_models)):
        keys = rec.keys(i)
        assert keys.dtype == np.int32 and np.array_equal(keys, om.keys), (MODELS[i], keys.shape, om.keys.shape)
        info = rec.model_info(i)
        assert info["n_keys"] == om.n_keys and info["n_rows"] == det.info()["n_ref"] == MODELS[i][2]
        assert info["n_bins"] == [om.n_a, om.n_a, om.n_a, om.n_d], (info, om.n_a, om.n_d)
        words = (om.n_a ** 3 * om.n_d + 31) // 32
        assert info["bytes"] >= 4 * words
        # the 72-bin model's set (38^3 x n_d bits) does not fit LDS twice beside the rows: it is read from global memory
        assert info["in_lds"] == (1 if 4 * words <= 48 * 1024 else 0) == (0 if MODELS[i][1] == 72 else 1), (MODELS[i], info)
    assert (oracle_models[0].keys == INT32_MIN).any(), "the turned box has no NaN-angle key: the fixture lost its point"
    n = np.zeros(1, np.int32)
    assert _capi.lib().ppf_recognizer_keys(rec._ptr, 0, None, 0, n.ctypes.data_as(_capi.C.POINTER(_capi.C.c_int))) == _capi.PPF_ERR_CAPACITY
    assert int(n[0]) == oracle_models[0].n_keys


def test_every_proposal_equals_the_oracle_in_one_call_and_alone(rec, oracle_models, proposals):
    clouds = [c for _, c in proposals]
    ranked, n_used, counts, st = check_call(rec, oracle_models, clouds, top=4)
    names = [n for n, _ in proposals]
    assert int(n_used[names.index("cylinder513")]) == 257  # stride 2 at max_rows 512
    assert int(n_used[names.index("nonfinite")]) == 126 and int(n_used[names.index("null")]) == 0
    assert len(ranked[names.index("null")]) == 0 and len(ranked[names.index("empty")]) == 0
    par = names.index("parallel")
    assert counts[par, 0, 0] > 0, "pairs of exactly parallel normals (a NaN angle) are known to the turned box"
    # each proposal alone gives what it gave in the frame; a repeated call gives the same bytes
    again = rec.recognize([None if c is None else DeviceCloud.upload(c) for c in clouds], dict(top=4), return_counts=True)
    assert np.array_equal(again[1], n_used) and again[2].tobytes() == counts.tobytes()
    for i, c in enumerate(clouds):
        one = rec.recognize([None if c is None else DeviceCloud.upload(c)], dict(top=4), return_counts=True)
        assert int(one[1][0]) == int(n_used[i]) and one[2][0].tobytes() == counts[i].tobytes(), names[i]
        assert one[0][0].tobytes() == ranked[i].tobytes() == again[0][i].tobytes(), names[i]


def test_max_rows_sets_the_stride(rec, oracle_models, proposals):
    cloud = dict(proposals)["cylinder513"]
    for max_rows in (2, 100, 512, 513, 2048):
        _, n_used, _, _ = check_call(rec, oracle_models, [cloud], max_rows=max_rows)
        s = -(-513 // max_rows)
        assert int(n_used[0]) == -(-513 // s)


def test_eight_models_and_mixed_steps(proposals):
    clouds = [dict(proposals)[n] for n in ("torus300", "bottle260", "box65", "coincident")]
    # the reference's distance step, 0.025 of the diameter: 17^3 x 41 bits, 25 KB a model
    eight = [train(k, 30, 150 + 20 * i, step=0.025, seed=10 + i) for i, k in enumerate(K.KINDS + K.KINDS)]
    r8 = Recognizer(eight)
    assert sum(r8.model_info(i)["bytes"] for i in range(8)) > 160 * 1024  # more bitmaps than one CU's LDS holds
    check_call(r8, [R.Model.from_detector(d) for d in eight], clouds, top=8)
    mixed = [train("box", 30, 200), train("torus", 72, 180, step=0.08), train("bottle", 20, 260, step=0.03), train("cylinder", 45, 220, key_equality=1)]
    rm = Recognizer(mixed)
    assert len({rm.model_info(i)["n_bins"][0] for i in range(4)}) == 4 and {rm.model_info(i)["in_lds"] for i in range(4)} == {0, 1}
    check_call(rm, [R.Model.from_detector(d) for d in mixed], clouds, top=4)


def test_gates_top_and_the_tie_rule(dets, oracle_models, proposals):
    twice = Recognizer([dets[3], dets[1], dets[3]])  # the same model at 0 and 2: equal scores, the lower index first
    om = [oracle_models[3], oracle_models[1], oracle_models[3]]
    cloud = dict(proposals)["bottle260"]
    ranked, _, counts, _ = check_call(twice, om, [cloud], top=3)
    assert np.array_equal(counts[0, 0], counts[0, 2]) and ranked[0]["score"][0] > 0
    order = [int(m) for m in ranked[0]["model"]]
    assert order.index(0) + 1 == order.index(2)
    best = float(ranked[0]["score"][0])
    assert [int(m) for m in check_call(twice, om, [cloud], top=1)[0][0]["model"]] == order[:1]
    assert len(check_call(twice, om, [cloud], top=3, min_score=best)[0][0]) >= 1       # the bound itself passes
    assert len(check_call(twice, om, [cloud], top=3, min_score=np.nextafter(best, 2.0))[0][0]) == 0  # clutter
    prec = sorted(float(p) for p in ranked[0]["precision"])
    got = check_call(twice, om, [cloud], top=3, min_precision=prec[-1])[0][0]
    assert len(got) >= 1 and all(float(p) >= prec[-1] for p in got["precision"])


def test_a_darboux_model_is_refused():
    darboux = train("cylinder", 30, 150, feature=_capi.PPF_FEATURE_DARBOUX)
    with pytest.raises(_capi.PPFError) as e:
        Recognizer([train("box", 30, 150), darboux])
    assert e.value.status == _capi.PPF_ERR_INVALID and "DARBOUX" in str(e.value)


def test_one_wait_and_launches_that_do_not_depend_on_the_frame(rec, proposals):
    view = dict(proposals)["torus300"]
    one = rec.recognize([DeviceCloud.upload(view)], return_stats=True)[1]
    many = rec.recognize([DeviceCloud.upload(K.thin(view, 40 + 7 * i, seed=i)) for i in range(40)], return_stats=True)[1]
    none = rec.recognize([], return_stats=True)[1]
    assert one["n_host_syncs"] == many["n_host_syncs"] == none["n_host_syncs"] == 1
    assert one["n_launches"] == many["n_launches"] == none["n_launches"] == 2
    assert many["n_clouds"] == 40 and one["ms_wall"] > 0


def test_models_of_untouched_rows_name_all_four_solids():
    """recognition models trained presampled on one untouched row per voxel (0.06 of the diameter: 420 / 329 / 273 / 263 rows):
    the device names a noisy one-sided view of each solid, the box included, and equals the oracle"""
    dets = [PPF3DDetector(0.06, 0.05).trainModel(K.voxel_pick(K.solid(k), 0.06), presampled=True) for k in K.KINDS]
    views = [K.thin(K.one_sided_view(K.solid(k), 1000 * i), 400, seed=i) for i, k in enumerate(K.KINDS)]
    ranked = check_call(Recognizer(dets), [R.Model.from_detector(d) for d in dets], views, max_rows=400)[0]
    for i, rows in enumerate(ranked):
        assert int(rows["model"][0]) == i and rows["score"][1] <= 0.85 * rows["score"][0], (K.KINDS[i], rows)  # the conditions' bound


def test_recognize_frame_names_views_of_two_solids():
    cp = CloudProcessor()
    cp.LoadSingleModel(K.thin(K.solid("torus"), 6000, seed=1), "torus")
    cp.LoadSingleModel(K.solid("bottle"), "bottle")
    cp.TrainDetector(0.05, 0.05)
    views = [K.one_sided_view(K.solid("bottle"), 7), K.one_sided_view(K.solid("torus"), 8), np.zeros((0, 6), np.float32)]
    cp.object_mats = [DeviceCloud.upload(v) for v in views]  # what PrepareFrame leaves: one resident cloud per detection
    cp.edge_mats = [None] * len(views)
    labels = cp.RecognizeFrame(top=2, max_rows=400)
    assert labels == ["bottle", "torus", None]
    assert [c[0] for c in cp.frame_candidates[0]] == ["bottle", "torus"] and cp.frame_candidates[2] == []
    label, score, precision, recall = cp.frame_candidates[1][0]
    assert label == "torus" and score == precision * recall and 0 < score <= 1
    assert cp.recognize_stats["n_host_syncs"] == 1 and cp.recognize_stats["n_models"] == 2
    assert cp.RecognizeFrame(top=1, min_score=2.0) == [None, None, None]  # no score exceeds 1
