"""The model file on the CPU: tests/golden/tiny_model.ppf (the saved model of `tiny_cloud()` below, trained once on a
device) goes through ppf_model_check_file whole and with one patch per validation exit, and through
ppf_debug_model_row_groups, whose group records are checked against the rules stated above `row_groups` in
csrc/ppf_model_host.h.  No test here needs a device; tests/test_gpu_model_file.py trains the same cloud again."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN
from yolo_ppf_pose_estimation_amd import _capi
from yolo_ppf_pose_estimation_amd._capi import lib

FIXTURE = os.path.join(GOLDEN, "tiny_model.ppf")
SAMPLING, DISTANCE, MAX_TILE_REFS = 0.25, 0.05, 36  # a coarse distance step: many pairs per key; 70 rows in two tiles

# constants of csrc/ppf_core.h, ppf_match_kernels.h and ppf_train_kernels.h that the file's records are made of
AGG_Q, GROUP_CELLS, MIN_RECORDS, AGG_CHUNK, GROUP_X = 64, 4, 32, 1024, 8
ROW_CODE_MASK, ROW_X_SHIFT, ROW_Q_SHIFT, ROW_Q_MASK = 0x3FFFF, 18, 23, 127
CELLS_FREE = AGG_Q * 0x01010101


def tiny_cloud():
    """An 8 x 8 planar grid with equal normals (many pairs share a key) and six points off the plane (keys of their own)."""
    rng = np.random.default_rng(34)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2)
    plane = np.zeros((64, 6), dtype=np.float32)
    plane[:, :2] = g * 0.01
    plane[:, 5] = 1.0
    extra = np.zeros((6, 6), dtype=np.float32)
    extra[:, :3] = rng.uniform([0.0, 0.0, 0.005], [0.07, 0.07, 0.03], size=(6, 3))
    nrm = rng.normal(size=(6, 3))
    extra[:, 3:] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([plane, extra]), dtype=np.float32)


def vote_guard(A):
    return 64 + 2 * ((A + 1) | 1)


def first_real(A):
    """Row codes below this name the guard words: padding entries."""
    return (vote_guard(A) - A) * 4


def records_for(entries):
    return 32 * (entries // 64) + min(32, entries % 64)


class Image:
    """The sections of a model file (include/ppf_hip.h: ppf_model_save), offsets from ctypes.sizeof of the two structs."""

    def __init__(self, raw: bytes):
        self.raw = bytes(raw)
        self.o_params = 8 + 8  # magic, build word {count-table cells, 0}
        self.o_info = self.o_params + C.sizeof(_capi.TrainParams)
        self.o_nrec = self.o_info + C.sizeof(_capi.ModelInfo)
        self.params = _capi.TrainParams.from_buffer_copy(self.raw, self.o_params)
        self.info = _capi.ModelInfo.from_buffer_copy(self.raw, self.o_info)
        self.n_records = struct.unpack_from("<Q", self.raw, self.o_nrec)[0]
        I = self.info
        self.nb, self.T, self.A = I.n_buckets, I.n_tiles, I.num_angles
        self.o_sampled = self.o_nrec + 8
        self.o_slotmap = self.o_sampled + I.n_ref * 24
        self.words = (I.slots + 63) // 64
        self.o_boff = self.o_slotmap + self.words * 16
        self.o_bslot = self.o_boff + self.T * (self.nb + 1) * 4
        self.o_rec = self.o_bslot + self.nb * 4
        self.size = self.o_rec + self.n_records * 16
        self.slotmap = np.frombuffer(self.raw, np.uint32, self.words * 4, self.o_slotmap).reshape(-1, 4)
        self.boff = np.frombuffer(self.raw, np.uint32, self.T * (self.nb + 1), self.o_boff).reshape(self.T, self.nb + 1)
        self.records = np.frombuffer(self.raw, np.uint32, self.n_records * 4, self.o_rec).reshape(-1, 4)

    def field(self, struct_offset, cls, name):
        return struct_offset + getattr(cls, name).offset

    def buckets(self):
        """(tile, bucket, first record, records) of every (tile, bucket)"""
        for t in range(self.T):
            for b in range(self.nb):
                yield t, b, int(self.boff[t, b]), int(self.boff[t, b + 1] - self.boff[t, b])

    def slot_codes(self, off, cnt):
        """The row codes of a bucket's record slots (padding included), any order"""
        return self.records[off:off + cnt, :2].reshape(-1)


def fixture_facts(img: Image):
    """What the fixture must exercise (checked before it was committed and again by test_fixture_exercises_the_validator)."""
    sizes = [cnt for _, _, _, cnt in img.buckets()]
    big_group = 0
    for _, _, off, cnt in img.buckets():
        if cnt >= MIN_RECORDS:
            codes = img.slot_codes(off, cnt) & ((1 << ROW_Q_SHIFT) - 1)
            big_group = max(big_group, int(np.unique(codes, return_counts=True)[1].max()))
    return {"n_ref": img.info.n_ref, "n_tiles": img.T, "n_buckets": img.nb, "n_records": img.n_records,
            "largest_bucket": max(sizes), "smallest_nonempty": min(s for s in sizes if s), "eligible": sum(s >= MIN_RECORDS for s in sizes),
            "largest_group": big_group, "bytes": len(img.raw)}


# ---- the fixture and the validator -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw():
    with open(FIXTURE, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def img(raw):
    return Image(raw)


def check_bytes(tmp_path, data):
    p = tmp_path / "m.ppf"
    p.write_bytes(bytes(data))
    return lib().ppf_model_check_file(str(p).encode())


def test_fixture_is_a_valid_model_file(raw, img, tmp_path):
    assert len(raw) == img.size < 100_000
    assert lib().ppf_model_check_file(FIXTURE.encode()) == _capi.PPF_OK
    assert check_bytes(tmp_path, raw) == _capi.PPF_OK


def test_fixture_exercises_the_validator(img):
    """Two tiles (the tile-start check and the CSR chaining are live), a bucket that votes through count tables with a
    (row, X) group of more than four entries, a bucket that does not, a bucket whose dealing order crosses a block of 64."""
    facts = fixture_facts(img)
    assert 48 <= facts["n_ref"] <= 96 and facts["n_tiles"] == 2
    assert facts["eligible"] >= 1 and facts["largest_group"] > GROUP_CELLS
    assert 0 < facts["smallest_nonempty"] < MIN_RECORDS and facts["largest_bucket"] > 32
    assert (img.params.presampled, img.params.max_tile_refs) == (1, MAX_TILE_REFS)
    assert (img.params.relative_sampling_step, img.params.relative_distance_step) == (SAMPLING, DISTANCE)
    np.testing.assert_array_equal(np.frombuffer(img.raw, np.float32, img.info.n_ref * 6, img.o_sampled).reshape(-1, 6), tiny_cloud())


def _set(raw, offset, fmt, value):
    out = bytearray(raw)
    struct.pack_into(fmt, out, offset, value)
    return out


def _patches(img):
    """(exit's text, patched bytes): every patch reaches its own exit; a field the size sum reads is patched in the body."""
    raw, I = img.raw, img.info
    P, M = _capi.TrainParams, _capi.ModelInfo
    par = lambda name, fmt, v: _set(raw, img.field(img.o_params, P, name), fmt, v)
    inf = lambda name, fmt, v: _set(raw, img.field(img.o_info, M, name), fmt, v)
    N = I.n_ref
    yield "magic", _set(raw, 0, "<B", raw[0] ^ 1)
    yield "written by a build with another count-table cell count", _set(raw, 8, "<I", 48)
    yield "written by a build with another count-table cell count", _set(raw, 12, "<I", 1)
    yield "header", raw[:12]
    yield "header", raw[:img.o_nrec + 4]
    yield "n_ref", inf("n_ref", "<i", 1)
    yield "n_ref", inf("n_ref", "<i", 70000)
    yield "steps", inf("distance_step", "<d", 0.0)
    yield "steps", inf("num_angles", "<i", 0)
    yield "steps", inf("diameter", "<d", float("inf"))
    yield "key_equality", par("key_equality", "<i", 7)
    yield "feature", par("feature", "<i", 7)
    yield "angle step too fine for the key table", inf("angle_step", "<d", 0.002)
    yield "slots", inf("slots", "<I", I.slots * 2)
    yield "num_angles", inf("num_angles", "<i", I.num_angles - 1)
    yield "tiles", inf("n_tiles", "<i", 3)
    yield "tiles", inf("tile_refs", "<i", I.tile_refs - 1)
    one_tile = bytearray(inf("n_tiles", "<i", 1))
    struct.pack_into("<i", one_tile, img.field(img.o_info, M, "tile_refs"), 100000)
    yield "tile does not fit this build's LDS accumulator", one_tile
    yield "n_buckets", inf("n_buckets", "<I", I.slots + 1)
    yield "n_entries", inf("n_entries", "<Q", N * N + N + 1)
    yield "n_records", _set(raw, img.o_nrec, "<Q", 0xFFFFFFFF)
    yield "file size does not match its header", raw[: len(raw) // 2]
    yield "file size does not match its header", raw + b"\0" * 16
    yield "file size does not match its header", _set(raw, img.o_nrec, "<Q", img.n_records + 1)
    yield "sampled cloud", _set(raw, img.o_sampled + 4 * 7, "<f", float("nan"))
    yield "slot map ranks", _set(raw, img.o_slotmap + 8, "<I", 1)
    lo = int(img.slotmap[-1, 0])
    free = next(k for k in range(32) if not lo >> k & 1)  # one more slot in use in the last word: every rank still holds
    yield "slot map population", _set(raw, img.o_slotmap + 16 * (img.words - 1), "<I", lo | 1 << free)
    yield "bucket slots", _set(raw, img.o_bslot, "<I", I.slots)
    row1 = img.o_boff + 4 * (img.nb + 1)
    yield "bucket offsets (tile start)", _set(raw, row1, "<I", int(img.boff[1, 0]) + 1)
    yield "bucket offsets (order)", _set(raw, img.o_boff + 4, "<I", 0xFFFFFFF0)
    yield "bucket offsets (total)", _set(raw, row1 + 4 * img.nb, "<I", img.n_records + 1)
    yield "record row", _set(raw, img.o_rec + 1, "<B", 0xFF)
    yield "record row", _set(raw, img.o_rec, "<B", raw[img.o_rec] | 2)
    yield "record cell", _set(raw, img.o_rec + 3, "<B", raw[img.o_rec + 3] | 0x3F)
    yield "record cell", _set(raw, img.o_rec + 7, "<B", raw[img.o_rec + 7] | 0x40)
    yield "record alpha", _set(raw, img.o_rec + 8, "<f", float("nan"))
    yield "record alpha", _set(raw, img.o_rec + 12, "<f", 3.5)
    halves = img.records[:, 0] & 1
    victim = None  # a bucket whose share of high-half rows spans >= 3 records: a low-half row in the middle of them
    for _, _, off, cnt in img.buckets():
        h = np.flatnonzero(halves[off:off + cnt] & (img.records[off:off + cnt, 0] & ROW_CODE_MASK >= first_real(img.A)))
        if len(h) >= 3:
            victim = off + int(h[1])
            break
    assert victim is not None
    yield "record halves (order)", _set(raw, img.o_rec + 16 * victim, "<B", raw[img.o_rec + 16 * victim] ^ 1)


def test_every_validation_exit_is_reached_by_its_own_patch(img, tmp_path):
    seen = set()
    for what, data in _patches(img):
        assert check_bytes(tmp_path, data) == _capi.PPF_ERR_IO, what
        assert f"({what})" in _capi.last_error(), (what, _capi.last_error())
        seen.add(what)
    assert len(seen) == 27  # every bad(...) of the validator but "seek" and "short read", which no file on a disk reaches


# ---- ppf_debug_model_row_groups ----------------------------------------------------------------------------------------------
def row_groups(data):
    """(status, group records [n, 4], grp_hdr [m, 2]) through the capacity protocol: NULL buffers report the need."""
    n, m = C.c_uint64(0), C.c_uint64(0)
    rc = lib().ppf_debug_model_row_groups(data, len(data), None, 0, None, 0, C.byref(n), C.byref(m))
    if rc != _capi.PPF_OK:
        return rc, None, None
    rec, hdr = np.zeros((n.value, 4), np.uint32), np.zeros((m.value, 2), np.uint32)
    rc = lib().ppf_debug_model_row_groups(data, len(data), rec.ctypes.data, n.value, hdr.ctypes.data, m.value, C.byref(n), C.byref(m))
    assert (n.value, m.value) == (len(rec), len(hdr))
    return rc, rec, hdr


def expected_groups(codes):
    """The groups of a bucket's record slots by the rules: slots sorted by (row and X, cell), every run of equal (row, X)
    cut into groups of up to four cells; {used slots: sorted [(code, cell bytes with the free slots naming AGG_Q)]}."""
    key, cell = codes & ((1 << ROW_Q_SHIFT) - 1), (codes >> ROW_Q_SHIFT) & ROW_Q_MASK
    by_used = {u: [] for u in range(1, GROUP_CELLS + 1)}
    for k in np.unique(key):
        cells = np.sort(cell[key == k]).tolist()
        for f in range(0, len(cells), GROUP_CELLS):
            part = cells[f:f + GROUP_CELLS]
            word = sum((part[i] if i < len(part) else AGG_Q) << 8 * i for i in range(GROUP_CELLS))
            by_used[len(part)].append((int(k), word))
    return {u: sorted(v) for u, v in by_used.items()}


def test_row_groups_of_the_fixture_follow_their_rules(raw, img):
    rc, rec, hdr = row_groups(raw)
    assert rc == _capi.PPF_OK and len(hdr) == img.n_records // 32 + 1
    named, base, eligible = set(), 0, 0
    for _, _, off, cnt in img.buckets():
        if cnt < MIN_RECORDS:
            continue  # votes directly: no group records, no slice (checked below: every entry of grp_hdr no chunk names is zero)
        eligible += 1
        want = expected_groups(img.slot_codes(off, cnt))
        n_grp = sum(len(v) for v in want.values())
        n_rec = records_for(n_grp)
        # the slots of the bucket's group records in dealing order: position j = record 32*(j/64) + j%32, slot (j%64)/32
        pos = [(32 * (j // 64) + j % 32, (j % 64) // 32) for j in range(64 * ((n_rec + 31) // 32))]
        slots = [(int(rec[base + r, s]), int(rec[base + r, 2 + s])) for r, s in pos if r < n_rec]
        assert len(slots) == 2 * n_rec >= n_grp
        at = 0
        for used in range(GROUP_CELLS, 0, -1):  # records with more used slots first; no group mixes (row, X): one code each
            assert sorted(slots[at:at + len(want[used])]) == want[used], (off, used)
            at += len(want[used])
        for code, cells in slots[n_grp:]:  # free slots: the all-zero row AGG_Q of a padding row in the guard words
            assert cells == CELLS_FREE and code >> ROW_X_SHIFT == GROUP_X and (code & ROW_CODE_MASK) < 256 and code & 3 == 0
        # the bucket's chunks of at least 32 pair records share its group records out in whole blocks of 32
        first = base
        for k in range(0, cnt, AGG_CHUNK):
            if min(AGG_CHUNK, cnt - k) < 32:
                continue
            h = (off + k) >> 5
            assert h not in named
            named.add(h)
            assert int(hdr[h, 0]) == first and (first - base) % 32 == 0
            first += int(hdr[h, 1])
        assert first == base + n_rec
        base += n_rec
    assert eligible >= 1 and base == len(rec)
    rest = np.ones(len(hdr), bool)
    rest[sorted(named)] = False
    assert not hdr[rest].any()


def test_row_groups_entry_capacity_and_corrupt_bytes(raw, img):
    n, m = C.c_uint64(0), C.c_uint64(0)
    f = lib().ppf_debug_model_row_groups
    assert f(raw, len(raw), None, 0, None, 0, C.byref(n), C.byref(m)) == _capi.PPF_OK and n.value > 0 and m.value > 0
    rec, hdr = np.zeros((n.value, 4), np.uint32), np.zeros((m.value, 2), np.uint32)
    need = (n.value, m.value)
    for cap_r, cap_h in ((need[0] - 1, need[1]), (need[0], need[1] - 1)):
        n.value = m.value = 0
        assert f(raw, len(raw), rec.ctypes.data, cap_r, hdr.ctypes.data, cap_h, C.byref(n), C.byref(m)) == _capi.PPF_ERR_CAPACITY
        assert (n.value, m.value) == need and not rec.any() and not hdr.any()
    assert f(raw, len(raw), rec.ctypes.data, need[0], None, 0, C.byref(n), C.byref(m)) == _capi.PPF_OK and rec.any() and not hdr.any()
    assert f(None, len(raw), None, 0, None, 0, C.byref(n), C.byref(m)) == _capi.PPF_ERR_INVALID
    assert f(raw, len(raw), None, 0, None, 0, None, C.byref(m)) == _capi.PPF_ERR_INVALID
    assert f(raw, 0, None, 0, None, 0, C.byref(n), C.byref(m)) == _capi.PPF_ERR_IO
    bad = _set(raw, img.o_rec + 1, "<B", 0xFF)
    assert row_groups(bytes(bad))[0] == _capi.PPF_ERR_IO and "(record row)" in _capi.last_error()
    assert row_groups(raw[: len(raw) // 2])[0] == _capi.PPF_ERR_IO and "(file size does not match its header)" in _capi.last_error()
