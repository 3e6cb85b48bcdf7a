"""A numpy restatement of DESIGN.md §16 (ppf_select_frame) on top of render_oracle.zbuffer: per hypothesis the drawn and
supported pixel sets, the explained share, the rank key and the gate, then the greedy pass over the eligible hypotheses and
the depth / label images of the selected ones.  Counts are integers and every float is the fixed fp32 / fp64 expression the
kernels evaluate, so the device's bytes are expected, not approximations of them."""
import hashlib

import numpy as np

import render_oracle as R

NONE, SELECTED, GATED, SUPPRESSED = 0, 1, 2, 3
INFO = np.dtype([("status", "<i4"), ("rank", "<i4"), ("suppressed_by", "<i4"), ("n_drawn", "<i4"), ("n_supported", "<i4"),
                 ("n_overlap", "<i4"), ("explained", "<f4"), ("key", "<f4"), ("reserved", "<i4", (4,))])
DEFAULTS = dict(depth_tol=0.01, max_overlap=0.25, min_score=0.0, min_pixels=1)


def pixel_sets(o, depth, intr, radius, depth_tol, cache=None):
    """steps 1-2 for the moved rows o of one hypothesis: (z-buffer bits, flat indices of D, flat indices of S); `cache`
    (a dict) keeps the z-buffer of (rows, image, radius) between calls that differ in the other parameters"""
    rows, cols = depth.shape
    key = (hashlib.sha1(o.tobytes()).digest(), rows, cols, tuple(float(v) for v in intr), float(np.float32(radius)))
    if cache is not None and key in cache:
        zb = cache[key]
    else:
        zb = R.zbuffer(o, rows, cols, intr, radius).reshape(-1)
        if cache is not None:
            cache[key] = zb
    drawn = np.flatnonzero(zb != R.EMPTY32)
    d = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1)[drawn]
    z = zb[drawn].view(np.float32)
    with np.errstate(all="ignore"):
        ok = np.isfinite(d) & (d > 0) & (np.abs(d - z) <= np.float32(depth_tol))   # the difference in fp32
    return zb, drawn, drawn[ok]


def explained_share(n_supported, n_drawn):
    return np.float32(float(n_supported) / float(n_drawn)) if n_drawn > 0 else np.float32(0)


def select(hyps, n_flat, depth, intr, radius, depth_tol=0.01, max_overlap=0.25, min_score=0.0, min_pixels=1, keys=None,
           cache=None):
    """hyps: (j, moved rows) per hypothesis, j = i * top + k ascending; n_flat = n_dets * top; keys: None (rank by
    explained) or a mapping / array j -> score.  Returns a dict: info (INFO rows, zero where no hypothesis), selected (n_flat
    flat indices in selection order, then -1), n_selected, n_eligible, depth and label images."""
    rows, cols = depth.shape
    info = np.zeros(n_flat, dtype=INFO)
    zbs, sup = {}, {}
    for j, o in hyps:
        zbs[j], drawn, sup[j] = pixel_sets(o, depth, intr, radius, depth_tol, cache)
        r = info[j]
        r["rank"] = r["suppressed_by"] = -1
        r["n_drawn"], r["n_supported"] = drawn.size, sup[j].size
        r["explained"] = explained_share(sup[j].size, drawn.size)
        r["key"] = np.float32(keys[j]) if keys is not None else r["explained"]
        with np.errstate(invalid="ignore"):
            eligible = bool(r["key"] >= np.float32(min_score)) and int(r["n_supported"]) >= int(min_pixels)
        r["status"] = SELECTED if eligible else GATED
    order = sorted((j for j, _ in hyps if info[j]["status"] == SELECTED), key=lambda j: (-float(info[j]["key"]), j))
    limit = float(np.float32(max_overlap))
    chosen = []
    for j in order:
        for a in chosen:   # in selection order: the first conflict is the earliest-selected one
            ov = int(np.intersect1d(sup[a], sup[j], assume_unique=True).size)
            if float(ov) > limit * float(min(int(info[a]["n_supported"]), int(info[j]["n_supported"]))):
                info[j]["status"], info[j]["suppressed_by"], info[j]["n_overlap"] = SUPPRESSED, a, ov
                break
        else:
            info[j]["rank"] = len(chosen)
            chosen.append(j)
    frame = np.full(rows * cols, R.EMPTY64, dtype=np.uint64)
    for j in chosen:
        np.minimum(frame, (zbs[j].astype(np.uint64) << np.uint64(32)) | np.uint64(j), out=frame, where=zbs[j] != R.EMPTY32)
    empty = frame == R.EMPTY64
    img = (frame >> np.uint64(32)).astype(np.uint32).view(np.float32)
    img[empty] = 0
    label = (frame & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    label[empty] = -1
    selected = np.full(n_flat, -1, dtype=np.int32)
    selected[:len(chosen)] = chosen
    return dict(info=info, selected=selected, n_selected=len(chosen), n_eligible=len(order), depth=img.reshape(rows, cols),
                label=label.reshape(rows, cols), supported=sup)
