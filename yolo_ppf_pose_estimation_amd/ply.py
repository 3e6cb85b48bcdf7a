"""Minimal PLY I/O for N x 6 float32 clouds (x y z nx ny nz).

Mirrors the helpers the reference's driver takes from OpenCV's ppf_match_3d namespace:
``loadPLYSimple(path, withNormals)`` (/root/reference/src/YOLO_cropping_ppf_test.cpp:114) and
``writePLY(cloud, path)`` (:127).  ASCII vertex lists only, which is what the reference's model
file (data/bottle_remesh_meter_normalized.ply, header lines 1-13) uses.  ``load_ply_mesh`` / ``write_ply_mesh`` add the
faces, for ``DeviceCloud.from_mesh`` and ``CloudProcessor.LoadMeshModel``.
"""
from __future__ import annotations

import numpy as np


def load_ply_simple(path: str, with_normals: bool = True) -> np.ndarray:
    """Return an (N, 6) or (N, 3) float32 array from an ASCII PLY vertex list."""
    with open(path, "rb") as fh:
        n_vertex = None
        n_props = 0
        in_vertex = False
        while True:
            line = fh.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            tok = line.decode("ascii", "replace").split()
            if not tok:
                continue
            if tok[0] == "format" and tok[1] != "ascii":
                raise ValueError(f"{path}: only ascii PLY is supported")
            if tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    n_vertex = int(tok[2])
            elif tok[0] == "property" and in_vertex:
                n_props += 1
            elif tok[0] == "end_header":
                break
        if n_vertex is None:
            raise ValueError(f"{path}: no vertex element")
        data = np.loadtxt(fh, dtype=np.float64, max_rows=n_vertex, ndmin=2)
    need = 6 if with_normals else 3
    if data.shape[1] < need or n_props < need:
        raise ValueError(f"{path}: {data.shape[1]} columns, need {need}")
    out = np.ascontiguousarray(data[:, :need], dtype=np.float32)
    if with_normals:
        # loadPLYSimple re-normalises the normals it reads
        nrm = np.linalg.norm(out[:, 3:6].astype(np.float64), axis=1)
        ok = nrm > 1e-12
        out[ok, 3:6] = (out[ok, 3:6].astype(np.float64) / nrm[ok, None]).astype(np.float32)
    return out


def write_ply(cloud: np.ndarray, path: str) -> None:
    """Write an (N, 3|6) float cloud as ASCII PLY."""
    cloud = np.asarray(cloud)
    with_normals = cloud.shape[1] >= 6
    with open(path, "w") as fh:
        fh.write("ply\nformat ascii 1.0\n")
        fh.write(f"element vertex {cloud.shape[0]}\n")
        fh.write("property float x\nproperty float y\nproperty float z\n")
        if with_normals:
            fh.write("property float nx\nproperty float ny\nproperty float nz\n")
        fh.write("end_header\n")
        cols = 6 if with_normals else 3
        for row in cloud[:, :cols]:
            fh.write(" ".join(repr(float(np.float32(v))) for v in row) + "\n")


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_header(fh, path):
    """(format, [(element, count, [(property, type) | (property, (count type, item type))])]); fh is left at the body"""
    if fh.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, elements = None, []
    while True:
        line = fh.readline()
        if not line:
            raise ValueError(f"{path}: no end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: a property before any element")
            try:
                kind = (_PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]) if tok[1] == "list" else _PLY_TYPES[tok[1]]
            except KeyError as e:
                raise ValueError(f"{path}: unknown property type {e}") from None
            elements[-1][2].append((tok[-1], kind))
        elif tok[0] == "end_header":
            break
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: only ascii and binary_little_endian PLY are supported, not {fmt}")
    return fmt, elements


def _ply_rows(fmt, count, props, tokens, pos, buf, off):
    """one element's rows, each a list of its properties' values (a list property's value is a list)"""
    rows = []
    for _ in range(count):
        row = []
        for _, kind in props:
            if fmt == "ascii":
                if isinstance(kind, tuple):
                    n = int(tokens[pos])
                    row.append([float(t) for t in tokens[pos + 1:pos + 1 + n]])
                    if len(row[-1]) != n:
                        raise ValueError("the file ends inside a list")
                    pos += 1 + n
                else:
                    row.append(float(tokens[pos]))
                    pos += 1
            elif isinstance(kind, tuple):
                ct, it = np.dtype("<" + kind[0]), np.dtype("<" + kind[1])
                n = int(np.frombuffer(buf, ct, 1, off)[0])
                row.append(np.frombuffer(buf, it, n, off + ct.itemsize).tolist())
                off += ct.itemsize + n * it.itemsize
            else:
                dt = np.dtype("<" + kind)
                row.append(np.frombuffer(buf, dt, 1, off)[0].item())
                off += dt.itemsize
        rows.append(row)
    return rows, pos, off


def load_ply_mesh(path: str):
    """(vertices (N, 3 | 6) float32, triangles (M, 3) int32) of an ASCII or binary_little_endian PLY: the vertex element's
    x y z and, when all three are there, nx ny nz (other vertex properties are skipped); the face element's vertex_indices /
    vertex_index lists, polygons fanned from their first vertex.  A file without faces gives (0, 3) triangles."""
    with open(path, "rb") as fh:
        fmt, elements = _ply_header(fh, path)
        body = fh.read()
    tokens = body.split() if fmt == "ascii" else None
    pos = off = 0
    vertices, triangles = None, np.zeros((0, 3), dtype=np.int32)
    try:
        for name, count, props in elements:
            names = [p[0] for p in props]
            scalar = all(not isinstance(k, tuple) for _, k in props)
            if scalar and fmt == "ascii":
                table = np.array(tokens[pos:pos + count * len(props)], dtype=np.float64).reshape(count, len(props))
                pos += count * len(props)
            elif scalar:
                dt = np.dtype([(f"f{i}", "<" + k) for i, (_, k) in enumerate(props)])
                rec = np.frombuffer(body, dt, count, off)
                off += count * dt.itemsize
                table = np.stack([rec[f"f{i}"].astype(np.float64) for i in range(len(props))], axis=1) if props else np.zeros((count, 0))
            else:
                rows, pos, off = _ply_rows(fmt, count, props, tokens, pos, body, off)
                table = rows
            if name == "vertex":
                if not scalar or not all(c in names for c in "xyz"):
                    raise ValueError("the vertex element needs scalar x, y and z")
                cols = ["x", "y", "z"] + (["nx", "ny", "nz"] if all(c in names for c in ("nx", "ny", "nz")) else [])
                vertices = np.ascontiguousarray(table[:, [names.index(c) for c in cols]], dtype=np.float32)
            elif name == "face":
                li = [i for i, n in enumerate(names) if n in ("vertex_indices", "vertex_index")]
                if not li or scalar:
                    raise ValueError("the face element has no vertex_indices list")
                fans = []
                for row in table:
                    poly = [int(v) for v in row[li[0]]]
                    fans += [(poly[0], poly[i], poly[i + 1]) for i in range(1, len(poly) - 1)]
                triangles = np.array(fans, dtype=np.int32).reshape(-1, 3)
    except (ValueError, IndexError) as e:
        raise ValueError(f"{path}: {e}") from None
    if vertices is None:
        raise ValueError(f"{path}: no vertex element")
    if len(triangles) and (triangles.min() < 0 or triangles.max() >= len(vertices)):
        raise ValueError(f"{path}: a face index outside the {len(vertices)} vertices")
    return vertices, triangles


def write_ply_mesh(vertices: np.ndarray, triangles: np.ndarray, path: str) -> None:
    """Write (N, 3|6) float vertices and (M, 3) triangles as an ASCII PLY that load_ply_mesh and load_ply_simple read."""
    vertices, triangles = np.asarray(vertices), np.asarray(triangles).reshape(-1, 3)
    cols = 6 if vertices.shape[1] >= 6 else 3
    with open(path, "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\nelement vertex {vertices.shape[0]}\n")
        fh.write("property float x\nproperty float y\nproperty float z\n")
        if cols == 6:
            fh.write("property float nx\nproperty float ny\nproperty float nz\n")
        fh.write(f"element face {triangles.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
        for row in vertices[:, :cols]:
            fh.write(" ".join(repr(float(np.float32(v))) for v in row) + "\n")
        for t in triangles:
            fh.write(f"3 {int(t[0])} {int(t[1])} {int(t[2])}\n")


def transform_pc_pose(cloud: np.ndarray, pose: np.ndarray) -> np.ndarray:
    """ppf_match_3d::transformPCPose (/root/reference/src/YOLO_cropping_ppf_test.cpp:125):
    apply a 4x4 pose to points (with homogeneous divide) and rotate+renormalise normals."""
    cloud = np.asarray(cloud, dtype=np.float32)
    pose = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    out = cloud.copy()
    p = cloud[:, :3].astype(np.float64)
    ph = p @ pose[:3, :3].T + pose[:3, 3]
    w = p @ pose[3, :3].T + pose[3, 3]
    ok = np.abs(w) > 1e-12
    ph[ok] /= w[ok, None]
    out[:, :3] = ph.astype(np.float32)
    if cloud.shape[1] >= 6:
        n = cloud[:, 3:6].astype(np.float64) @ pose[:3, :3].T
        nrm = np.linalg.norm(n, axis=1)
        ok = nrm > 1e-12
        n[ok] /= nrm[ok, None]
        out[:, 3:6] = n.astype(np.float32)
    return out
