"""Mesh export: marching cubes on the GPU (csrc/mesh.hip, cnerf_marching_cubes_*), mesh cleanup on the GPU (csrc/mesh_clean.hip:
removal of small connected components, simplification by vertex clustering; csrc/mesh_decimate.hip: quadric edge-collapse decimation to a
face count) and a binary PLY writer.

The reference turns a density volume into a mesh with skimage.measure.marching_cubes on the host and writes it with plyfile
(nerf/renderer.py:128-196).  Here the surface is extracted by three passes on the device; the two counts are the only host read.
The table is crack-free for any input (csrc/gen_mc_tables.py); it is not skimage's Lewiner table, so vertex and triangle lists differ
from skimage's while describing the same isosurface.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import lib, check, ptr, stream, require_cuda


def _triple(v, name):
    t = tuple(float(x) for x in (v if np.ndim(v) else (v, v, v)))
    if len(t) != 3:
        raise ValueError(f"marching_cubes: {name} needs 3 values, got {len(t)}")
    return (C.c_float * 3)(*t)


def workspace_bytes(shape):
    nx, ny, nz = (int(s) for s in shape)
    out = C.c_uint64(0)
    check(lib.cnerf_marching_cubes_workspace_bytes(nx, ny, nz, C.byref(out)), "marching_cubes_workspace_bytes")
    return out.value


def marching_cubes(volume, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), normals=True):
    """Isosurface {volume == level} of a CUDA float32 tensor [X, Y, Z] (meshgrid('ij') order: Z fastest); a corner is inside when
    value >= level (NaN counts as outside).  -> (verts [V, 3] float32, faces [F, 3] int32, normals [V, 3] float32 or None), on the device.
    Vertex i of grid point (x, y, z) on axis a sits at origin + (idx + t) * spacing along a and origin + idx * spacing along the others;
    triangles wind (v1 - v0) x (v2 - v0) from inside to outside and the normals point the same way (towards lower values)."""
    require_cuda(volume)
    if volume.dim() != 3:
        raise ValueError(f"marching_cubes: volume must be [X, Y, Z], got {tuple(volume.shape)}")
    vol = volume.detach().contiguous().float()
    nx, ny, nz = vol.shape
    sp, org = _triple(spacing, "spacing"), _triple(origin, "origin")
    dev = vol.device
    nbytes = workspace_bytes(vol.shape)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    level = float(level)
    check(lib.cnerf_marching_cubes_count(ptr(vol), nx, ny, nz, level, ptr(ws), nbytes, ptr(counts), stream()), "marching_cubes_count")
    V, F = (int(c) & 0xffffffff for c in counts.cpu())                         # the one host read
    if V == 0xffffffff:
        raise ValueError(f"marching_cubes: the mesh of a {nx}x{ny}x{nz} volume has more than 2^31 - 1 vertices or triangles")
    verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
    nrm = torch.empty(V, 3, dtype=torch.float32, device=dev) if normals else None
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    check(lib.cnerf_marching_cubes_emit(ptr(vol), nx, ny, nz, level, org, sp, ptr(ws), nbytes, ptr(verts) if V else None,
                                        ptr(nrm) if V else None, ptr(faces) if F else None, V, F, stream()), "marching_cubes_emit")
    return verts, faces, nrm


def _mesh_args(verts, faces, normals, what):
    require_cuda(verts, faces, normals)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: verts and faces must be [V, 3] and [F, 3], got {tuple(verts.shape)} and {tuple(faces.shape)}")
    if normals is not None and tuple(normals.shape) != tuple(verts.shape):
        raise ValueError(f"{what}: normals must be [V, 3] like verts, got {tuple(normals.shape)}")
    v = verts.detach().contiguous().float()
    f = faces.detach().contiguous().to(torch.int32)
    n = None if normals is None else normals.detach().contiguous().float()
    return v, f, n


def _counts(counts, what):
    V, F, flags = (int(c) & 0xffffffff for c in counts.cpu())                  # the one host read
    if flags & 1:
        raise ValueError(f"{what}: a face index lies outside [0, V)")
    return V, F


def components_workspace_bytes(V, F):
    out = C.c_uint64(0)
    check(lib.cnerf_mesh_components_workspace_bytes(int(V), int(F), C.byref(out)), "mesh_components_workspace_bytes")
    return out.value


def remove_small_components(verts, faces, normals=None, min_faces=1, largest=False):
    """Drop the connected components (vertices joined by a face) with fewer than `min_faces` faces — and, with largest=True, every component
    but the one with the most faces (the one holding the smallest vertex index on a tie).  A vertex no face references is a 0-face component.
    CUDA tensors verts [V, 3], faces [F, 3] (int), normals [V, 3] or None.  Kept vertices and faces keep their order.
    -> (verts [V', 3] float32, faces [F', 3] int32, normals [V', 3] or None, old_index [V'] int32: input index of each output vertex).
    A face index outside [0, V) raises ValueError."""
    v, f, n = _mesh_args(verts, faces, normals, "remove_small_components")
    V, F = v.shape[0], f.shape[0]
    mf = int(min_faces)
    if mf < 0 or mf >= 2 ** 32:
        raise ValueError(f"remove_small_components: min_faces must be in [0, 2^32), got {min_faces}")
    dev = v.device
    nbytes = components_workspace_bytes(V, F)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    lg = 1 if largest else 0
    check(lib.cnerf_mesh_components_count(ptr(f) if F else None, V, F, mf, lg, ptr(ws), nbytes, ptr(counts), stream()),
          "mesh_components_count")
    V2, F2 = _counts(counts, "remove_small_components")
    vo = torch.empty(V2, 3, dtype=torch.float32, device=dev)
    no = torch.empty(V2, 3, dtype=torch.float32, device=dev) if n is not None else None
    fo = torch.empty(F2, 3, dtype=torch.int32, device=dev)
    old = torch.empty(V2, dtype=torch.int32, device=dev)
    check(lib.cnerf_mesh_components_emit(ptr(v) if V else None, ptr(n) if V and n is not None else None, V, ptr(f) if F else None, F, mf, lg,
                                         ptr(ws), nbytes, ptr(vo) if V2 else None, ptr(no) if V2 and no is not None else None,
                                         ptr(fo) if F2 else None, ptr(old) if V2 else None, V2, F2, stream()), "mesh_components_emit")
    return vo, fo, no, old


def cluster_grid(verts, cell, origin=None):
    """(origin float32 [3], cell float32 [3], grid (gx, gy, gz)) of simplify(): `origin` defaults to the vertices' minimum, and the grid
    reaches the cell of the maximum under simplify's float32 cell formula."""
    c = np.array(cell if np.ndim(cell) else (cell, cell, cell), dtype=np.float32).reshape(3)
    if not (np.isfinite(c).all() and (c > 0).all()):
        raise ValueError(f"simplify: cell must be finite and > 0, got {cell}")
    if verts.shape[0] == 0:
        o = np.zeros(3, np.float32) if origin is None else np.array(origin, dtype=np.float32).reshape(3)
        return o, c, (1, 1, 1)
    lo, hi = (t.cpu().numpy().astype(np.float32) for t in torch.aminmax(verts.detach().float(), dim=0))
    o = lo if origin is None else np.array(origin, dtype=np.float32).reshape(3)
    if not (np.isfinite(o).all() and np.isfinite(hi).all()):
        raise ValueError("simplify: origin and vertices must be finite")
    top = np.floor((hi - o) / c)
    g = tuple(int(max(t, 0.0)) + 1 for t in top)
    return o, c, g


def cluster_workspace_bytes(V, F, grid):
    out = C.c_uint64(0)
    check(lib.cnerf_mesh_cluster_workspace_bytes(int(V), int(F), (C.c_uint32 * 3)(*grid), C.byref(out)), "mesh_cluster_workspace_bytes")
    return out.value


def simplify(verts, faces, cell, normals=None, origin=None, grid=None):
    """Vertex clustering with a quadric representative (Lindstrom 2000) on a grid of cells of edge `cell` (scalar or per axis) from `origin`
    (default: the vertices' minimum) — grid = (gx, gy, gz) cells, by default enough to reach the vertices' maximum.  One output vertex per
    occupied cell, in linear cell order: the minimiser of the cell's face quadrics (clamped to the cell); normals = normalised mean of the
    members'.  Faces are mapped to clusters; faces with two equal clusters and repeats of an unordered cluster triple are dropped.
    -> (verts [K, 3] float32, faces [F', 3] int32, normals [K, 3] or None).  A face index outside [0, V) raises ValueError."""
    v, f, n = _mesh_args(verts, faces, normals, "simplify")
    V, F = v.shape[0], f.shape[0]
    o, c, g = cluster_grid(v, cell, origin)
    if grid is not None:
        g = tuple(int(x) for x in grid)
    if len(g) != 3 or min(g) < 1 or g[0] * g[1] * g[2] >= 2 ** 31:
        raise ValueError(f"simplify: the grid {g} needs 1 <= g and gx * gy * gz < 2^31 (a larger cell)")
    dev = v.device
    og, cg, gg = (C.c_float * 3)(*o.tolist()), (C.c_float * 3)(*c.tolist()), (C.c_uint32 * 3)(*g)
    nbytes = cluster_workspace_bytes(V, F, g)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    check(lib.cnerf_mesh_cluster_count(ptr(v) if V else None, V, ptr(f) if F else None, F, og, cg, gg, ptr(ws), nbytes, ptr(counts), stream()),
          "mesh_cluster_count")
    K, F2 = _counts(counts, "simplify")
    vo = torch.empty(K, 3, dtype=torch.float32, device=dev)
    no = torch.empty(K, 3, dtype=torch.float32, device=dev) if n is not None else None
    fo = torch.empty(F2, 3, dtype=torch.int32, device=dev)
    check(lib.cnerf_mesh_cluster_emit(ptr(v) if V else None, ptr(n) if V and n is not None else None, V, ptr(f) if F else None, F, og, cg, gg,
                                      ptr(ws), nbytes, ptr(vo) if K else None, ptr(no) if K and no is not None else None,
                                      ptr(fo) if F2 else None, K, F2, stream()), "mesh_cluster_emit")
    return vo, fo, no


def decimate_workspace_bytes(V, F):
    out = C.c_uint64(0)
    check(lib.cnerf_mesh_decimate_workspace_bytes(int(V), int(F), C.byref(out)), "mesh_decimate_workspace_bytes")
    return out.value


_DECIMATE_FLAGS = ((1, "a face index lies outside [0, V)"), (2, "an edge lies in more than two faces or two faces use it in one direction"),
                   (4, "a face repeats a vertex index"))


def decimate(verts, faces, target_faces, normals=None, rounds=None):
    """Quadric edge-collapse decimation (Garland & Heckbert 1997) on the device to `target_faces` faces, in parallel rounds of independent
    collapses (csrc/mesh_decimate.hip; the rules are in include/customnerf_hip.h).  The mesh must be edge-manifold and consistently oriented
    with no face repeating an index, as marching cubes and remove_small_components give; boundary vertices stay where they are, the genus is
    kept.  Stops at F <= target_faces (then F is target_faces or one less) or when no valid collapse is left (F stays above the target).
    CUDA tensors verts [V, 3], faces [F, 3] (int), normals [V, 3] or None.  -> (verts [V', 3] float32, faces [F', 3] int32 (surviving input
    faces in input order), normals [V', 3] (normals[old_index]) or None, old_index [V'] int32).  Unreferenced vertices are dropped.
    rounds: a list that receives counts (referenced vertices, faces, collapses) after each round.  Bad input raises ValueError."""
    v, f, n = _mesh_args(verts, faces, normals, "decimate")
    V, F = v.shape[0], f.shape[0]
    target = int(target_faces)
    if target < 0 or target >= 2 ** 32:
        raise ValueError(f"decimate: target_faces must be in [0, 2^32), got {target_faces}")
    dev = v.device
    nbytes = decimate_workspace_bytes(V, F)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)

    def read():
        r = [int(c) & 0xffffffff for c in counts.cpu()]                         # the one host read per call
        for bit, what in _DECIMATE_FLAGS:
            if r[3] & bit:
                raise ValueError(f"decimate: {what}")
        return r

    check(lib.cnerf_mesh_decimate_init(ptr(v) if V else None, V, ptr(f) if F else None, F, ptr(ws), nbytes, ptr(counts), stream()),
          "mesh_decimate_init")
    nv, nf, _, _ = read()
    while nf > target:
        check(lib.cnerf_mesh_decimate_round(V, nf, target, ptr(ws), nbytes, ptr(counts), stream()), "mesh_decimate_round")
        nv, nf, done, _ = read()
        if rounds is not None:
            rounds.append((nv, nf, done))
        if done == 0:
            break
    vo = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    no = torch.empty(nv, 3, dtype=torch.float32, device=dev) if n is not None else None
    fo = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    old = torch.empty(nv, dtype=torch.int32, device=dev)
    check(lib.cnerf_mesh_decimate_emit(ptr(n) if V and n is not None else None, V, nf, ptr(ws), nbytes, ptr(vo) if nv else None,
                                       ptr(no) if nv and no is not None else None, ptr(fo) if nf else None, ptr(old) if nv else None,
                                       nv, nf, stream()), "mesh_decimate_emit")
    return vo, fo, no, old


def _host(a, dtype):
    if a is None:
        return None
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def write_ply(path, verts, faces, normals=None, colors=None):
    """Binary little-endian PLY with the element / property names plyfile writes for the reference's records (renderer.py:172-185):
    vertex `x y z` float (+ `nx ny nz` float, + `red green blue` uchar), face `property list uchar int vertex_indices`.
    Accepts tensors (any device) or arrays: verts [V, 3], faces [F, 3], normals [V, 3], colors [V, 3] uint8."""
    v = _host(verts, np.float32).reshape(-1, 3)
    f = _host(faces, np.int32).reshape(-1, 3)
    n = _host(normals, np.float32)
    c = _host(colors, np.uint8)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if c is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(len(v), dtype=np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if n is not None:
        n = n.reshape(-1, 3)
        rec["nx"], rec["ny"], rec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if c is not None:
        c = c.reshape(-1, 3)
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("vertex_indices", "<i4", (3,))]))
    frec["n"] = 3
    frec["vertex_indices"] = f
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property {'float' if t == '<f4' else 'uchar'} {name}" for name, t in fields]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())

