"""Mesh export: marching cubes on the GPU (csrc/mesh.hip, cnerf_marching_cubes_*) and a binary PLY writer.

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

