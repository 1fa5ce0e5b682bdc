"""Mesh export: marching cubes on the GPU (csrc/mesh.hip, cnerf_marching_cubes_*) over a dense volume, or over the 8^3-point bricks around
the surface only (csrc/mesh_sparse.hip, cnerf_marching_cubes_sparse_*; sparse_volume finds the bricks from a field without evaluating the
whole lattice, and the mesh is the dense one bit for bit in another order), mesh cleanup on the GPU (csrc/mesh_clean.hip:
removal of small connected components, simplification by vertex clustering; csrc/mesh_decimate.hip: quadric edge-collapse decimation to a
face count; csrc/mesh_smooth.hip: Taubin smoothing and area-weighted vertex normals; csrc/mesh_holes.hip: the topology report — edges,
boundary loops, Euler characteristic, watertightness — and the filling of simple boundary loops), texture baking into a per-face-pair atlas on the GPU,
uniform or with cells sized by the faces' edges (csrc/mesh_texture.hip), or into an atlas of axis-projected charts (csrc/mesh_charts.hip), a rasteriser for previews of the exported mesh from a camera pose (csrc/mesh_raster.hip: visibility buffer and
shaded images), closest-point queries through a bounding-volume hierarchy with a surface sampler and the mesh-to-mesh distance built on them,
watertight ray casts through the same hierarchy and the per-vertex ambient occlusion built on them, the projection of a low-polygon mesh's
texels onto the full-resolution surface for baking colour and normal maps, the generalized winding number with the inside test, the
signed distance and the voxel remesh built on it (csrc/mesh_bvh.hip), welded vertices with tangent frames and
tangent-space normal maps through the same bake (csrc/mesh_tangent.hip, k_bake_tspace of csrc/mesh_bake.h), TSDF fusion of rendered or
rasterised depth maps into a volume whose zero level is the surface the views show (TSDFVolume, csrc/mesh_tsdf.hip), the colour of
texels and vertices blended from the rendered views that see them (ViewColors, csrc/mesh_view_colors.hip), a binary PLY writer,
an OBJ + MTL + PNG writer and a glTF 2.0 binary (.glb) writer.

The reference turns a density volume into a mesh with skimage.measure.marching_cubes on the host and writes it with plyfile
(nerf/renderer.py:128-196).  Here the surface is extracted by three passes on the device; the two counts are the only host read.
The table is crack-free for any input (csrc/gen_mc_tables.py); it is not skimage's Lewiner table, so vertex and triangle lists differ
from skimage's while describing the same isosurface.
"""
import ctypes as C
import math
import os
import struct
import zlib
from functools import cached_property

import numpy as np
import torch

from ._lib import lib, check, ptr, stream, require_cuda, query_u64


def _triple(v, name):
    t = tuple(float(x) for x in (v if np.ndim(v) else (v, v, v)))
    if len(t) != 3:
        raise ValueError(f"marching_cubes: {name} needs 3 values, got {len(t)}")
    return (C.c_float * 3)(*t)


def _bytes(name, *args):
    """cnerf_<name>_workspace_bytes(*args): the size of a pass's workspace"""
    return query_u64(getattr(lib, f"cnerf_{name}_workspace_bytes"), *args)


def _workspace(dev, name, *args):
    nbytes = _bytes(name, *args)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _p(t):
    """pointer of a tensor, None for no tensor or an empty one"""
    return ptr(t) if t is not None and t.numel() else None


_BAD_INDEX = ((1, "a face index lies outside [0, V)"),)
_DECIMATE_FLAGS = _BAD_INDEX + ((2, "an edge lies in more than two faces or two faces use it in one direction"),
                                (4, "a face repeats a vertex index"))


def _read(counts, what, flags):
    """The one host read of a call: the device counts as unsigned ints; their last entry holds the flag bits, and the first set one of
    `flags` ((bit, message), ...) raises ValueError."""
    r = [int(c) & 0xffffffff for c in counts.cpu()]
    for bit, msg in flags:
        if r[-1] & bit:
            raise ValueError(f"{what}: {msg}")
    return r


def _outputs(dev, V, F, normals, old_index=True):
    """(verts [V, 3], normals [V, 3] or None, faces [F, 3], old_index [V] or None), uninitialised"""
    return (torch.empty(V, 3, dtype=torch.float32, device=dev), torch.empty(V, 3, dtype=torch.float32, device=dev) if normals else None,
            torch.empty(F, 3, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev) if old_index else None)


def workspace_bytes(shape):
    return _bytes("marching_cubes", *(int(s) for s in shape))


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
    ws, nbytes = _workspace(dev, "marching_cubes", nx, ny, nz)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    level = float(level)
    check(lib.cnerf_marching_cubes_count(ptr(vol), nx, ny, nz, level, ptr(ws), nbytes, ptr(counts), stream()), "marching_cubes_count")
    V, F = (int(c) & 0xffffffff for c in counts.cpu())                         # the one host read
    if V == 0xffffffff:
        raise ValueError(f"marching_cubes: the mesh of a {nx}x{ny}x{nz} volume has more than 2^31 - 1 vertices or triangles")
    verts, nrm, faces, _ = _outputs(dev, V, F, normals, old_index=False)
    check(lib.cnerf_marching_cubes_emit(ptr(vol), nx, ny, nz, level, org, sp, ptr(ws), nbytes, _p(verts), _p(nrm), _p(faces), V, F, stream()),
          "marching_cubes_emit")
    return verts, faces, nrm


# ------------------------------------------------------------------------------------------------ brick-sparse extraction
BRICK = 8                                                                      # lattice points per brick and axis (csrc/mesh_sparse.hip)
_BRICK_POINTS = BRICK ** 3


class SparseVolume:
    """A lattice of `shape` points of which only some bricks of 8 x 8 x 8 points hold values (include/customnerf_hip.h, the sparse
    marching-cubes section): coords [n, 3] int32, unique and sorted; values [n, 512] float32, point (x, y, z) in brick
    (x >> 3, y >> 3, z >> 3) at ((x & 7) * 8 + (y & 7)) * 8 + (z & 7); nbr [n, 27] int32, the brick at every offset of {-1, 0, 1}^3 or -1.
    origin / spacing are 3 floats.  Counters of how it was made: `evaluations` field values asked for (probe lattice + bricks),
    `rounds` passes of the growth loop (the last one found nothing missing), `probe` the seeding stride."""

    def __init__(self, shape, origin, spacing, coords, values, nbr, evaluations=0, rounds=0, probe=1):
        self.shape = tuple(int(s) for s in shape)
        self.origin, self.spacing = tuple(float(x) for x in origin), tuple(float(x) for x in spacing)
        self.coords, self.values, self.nbr = coords, values, nbr
        self.evaluations, self.rounds, self.probe = int(evaluations), int(rounds), int(probe)

    @property
    def n_bricks(self):
        return int(self.coords.shape[0])


def sparse_workspace_bytes(n_bricks):
    return _bytes("marching_cubes_sparse", int(n_bricks))


def _brick_grid(shape):
    return tuple(-(-int(s) // BRICK) for s in shape)


def _brick_coords(keys, gb):
    """brick keys (bx * gby + by) * gbz + bz, int64 -> [n, 3] int64"""
    return torch.stack([keys // (gb[1] * gb[2]), (keys // gb[2]) % gb[1], keys % gb[2]], dim=1)


def _brick_offsets(dev):
    o = torch.arange(27, device=dev)
    return torch.stack([o // 9 - 1, (o // 3) % 3 - 1, o % 3 - 1], dim=1)        # slot (dx + 1) 9 + (dy + 1) 3 + dz + 1


def _around(keys, gb):
    """-> (keys of the 27 bricks around each brick [n, 27], whether each lies inside the brick grid [n, 27])"""
    c = _brick_coords(keys, gb)[:, None, :] + _brick_offsets(keys.device)[None]
    inside = ((c >= 0) & (c < torch.tensor(gb, device=keys.device))).all(-1)
    return (c[..., 0] * gb[1] + c[..., 1]) * gb[2] + c[..., 2], inside


def _find(keys, k):
    """position of every k in the sorted unique keys, and whether it is there"""
    if not keys.numel():
        return torch.zeros_like(k), torch.zeros_like(k, dtype=torch.bool)
    pos = torch.searchsorted(keys, k.clamp(min=0)).clamp(max=keys.numel() - 1)
    return pos, keys[pos] == k


def _brick_nbr(keys, gb):
    k, inside = _around(keys, gb)
    pos, found = _find(keys, k)
    return torch.where(found & inside, pos, torch.full_like(pos, -1)).to(torch.int32).contiguous()


def _brick_values(fetch, keys, gb, chunk):
    """values [n, 512] of the bricks `keys`: fetch(ijk [m, 3] int64 global lattice indices) -> [m] float32"""
    dev = keys.device
    loc = torch.arange(_BRICK_POINTS, device=dev)
    loc = torch.stack([loc >> 6, (loc >> 3) & 7, loc & 7], dim=1)
    out = torch.empty(keys.numel(), _BRICK_POINTS, dtype=torch.float32, device=dev)
    per = max(1, int(chunk) // _BRICK_POINTS)
    for s in range(0, keys.numel(), per):
        ijk = (_brick_coords(keys[s:s + per], gb)[:, None, :] * BRICK + loc[None]).reshape(-1, 3)
        out[s:s + per] = fetch(ijk).reshape(-1, _BRICK_POINTS)
    return out


def _probe_index(n, probe, dev):
    """the multiples of `probe` below n, plus the last index"""
    idx = list(range(0, n, probe))
    if idx[-1] != n - 1:
        idx.append(n - 1)
    return torch.tensor(idx, dtype=torch.int64, device=dev)


def _seed_keys(inside, pidx, probe, gb):
    """Keys of the seed bricks: brick b is one when the probe points with index in [8 b - probe, 8 b + 8 + probe] on every axis are not
    all on one side.  inside [Px, Py, Pz] bool (value >= level), pidx the three probe index lists."""
    def box_any(a):
        for ax in range(3):
            lo = torch.arange(gb[ax], device=a.device)[:, None] * BRICK
            m = ((pidx[ax][None] >= lo - probe) & (pidx[ax][None] <= lo + BRICK + probe)).float()
            a = (torch.tensordot(m, a.movedim(ax, 0), dims=1) > 0).float().movedim(0, ax)
        return a > 0
    seed = box_any(inside.float()) & box_any((~inside).float())
    return torch.nonzero(seed.reshape(-1)).reshape(-1)


def _sparse_count(values, coords, nbr, shape, level, want_state):
    """cnerf_marching_cubes_sparse_count -> (workspace, its bytes, counts [3] on the device, state [n] uint8 or None)"""
    dev, n = values.device, int(coords.shape[0])
    ws, nbytes = _workspace(dev, "marching_cubes_sparse", n)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    state = torch.empty(n, dtype=torch.uint8, device=dev) if want_state else None
    check(lib.cnerf_marching_cubes_sparse_count(ptr(values), ptr(coords), ptr(nbr), n, *shape, float(level), ptr(ws), nbytes, ptr(state),
                                                ptr(counts), stream()), "marching_cubes_sparse_count")
    return ws, nbytes, counts, state


def _grow(fetch, keys, shape, origin, spacing, level, chunk, max_rounds, evaluations, probe, what):
    """Seeds -> the SparseVolume at the fixed point of: mesh state of the bricks (the count pass), need = the 26 neighbours of the
    crossing bricks that are not there yet, fetch and merge them."""
    gb, dev = _brick_grid(shape), keys.device
    values = _brick_values(fetch, keys, gb, chunk)
    evaluations += values.numel()
    rounds = 0
    nbr = torch.empty(0, 27, dtype=torch.int32, device=dev)
    while keys.numel():
        if rounds >= max_rounds:
            raise ValueError(f"{what}: the surface's bricks were still growing after max_rounds={max_rounds} rounds")
        rounds += 1                                                             # a round: one count pass; the last finds nothing missing
        nbr = _brick_nbr(keys, gb)
        state = _sparse_count(values, _brick_coords(keys, gb).to(torch.int32).contiguous(), nbr, shape, level, True)[3]
        k, inside = _around(keys[(state & 1).bool()], gb)
        cand = torch.unique(k[inside])
        need = cand[~_find(keys, cand)[1]]
        if not need.numel():                                                    # (the host read of a round)
            break
        more = _brick_values(fetch, need, gb, chunk)
        evaluations += more.numel()
        keys, perm = torch.sort(torch.cat([keys, need]))
        values = torch.cat([values, more])[perm]
    return SparseVolume(shape, origin, spacing, _brick_coords(keys, gb).to(torch.int32).contiguous(), values.contiguous(), nbr,
                        evaluations=evaluations, rounds=rounds, probe=probe)


def _shape3(shape, what):
    s = tuple(int(x) for x in shape)
    if len(s) != 3 or min(s) < 2 or max(s) > 1 << 20:
        raise ValueError(f"{what}: shape must be 3 sizes in [2, 2^20], got {tuple(shape)}")
    return s


def sparse_volume(sigma_fn, shape, origin, spacing, level, probe=4, chunk=2 ** 21, max_rounds=64, device=None):
    """The bricks of a `shape` lattice that the isosurface {field == level} passes through, found without evaluating the whole lattice.
    sigma_fn(x [m, 3] float32 on the device) -> [m] values, elementwise; lattice point ijk sits at origin + ijk.float() * spacing, computed
    on the device in float32 (what NeRFRenderer.density_volume computes, so both ask the field at identical points).
    Seeding: the field on the probe lattice — the indices that are multiples of `probe` on each axis plus the last one; a brick is a seed
    when the probe values around it (index box [8 b - probe, 8 b + 8 + probe]^3) are not all on one side of `level`.  Growth: evaluate
    the seeds, then repeat: the count pass of marching_cubes_sparse says which bricks cross; their 26 neighbours that are missing are
    evaluated and merged; stop when none is missing (ValueError when max_rounds such rounds have not got there).  At that fixed point every crossing brick has
    all its neighbours, which is what marching_cubes_sparse needs, and every piece of surface connected — through cells whose corners
    lie on both sides — to something the seeding saw is covered, so the mesh equals marching_cubes of the full lattice.
    probe=1 examines every lattice point: nothing can be missed.  With probe=k only surface components that lie wholly between probe
    points — no probe point inside them or no probe point outside a hole — can be missed: the class of loss of an extraction at
    resolution / k, and nothing that is connected to a seen crossing is lost.
    -> SparseVolume; .evaluations counts the calls' points (probe lattice + 512 per brick)."""
    what = "sparse_volume"
    shape, probe = _shape3(shape, what), int(probe)
    if probe < 1:
        raise ValueError(f"{what}: probe must be >= 1, got {probe}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    org = torch.as_tensor(origin, dtype=torch.float32).reshape(3).to(dev)
    sp = torch.as_tensor(spacing, dtype=torch.float32).reshape(3).to(dev)

    def fetch(ijk):
        return sigma_fn((org + ijk.float() * sp).contiguous()).reshape(-1).float()

    pidx = [_probe_index(n, probe, dev) for n in shape]
    P = tuple(len(p) for p in pidx)
    n = P[0] * P[1] * P[2]
    inside = torch.empty(n, dtype=torch.bool, device=dev)
    for s in range(0, n, chunk):
        i = torch.arange(s, min(s + chunk, n), device=dev, dtype=torch.int64)
        ijk = torch.stack([pidx[0][i // (P[1] * P[2])], pidx[1][(i // P[2]) % P[1]], pidx[2][i % P[2]]], dim=1)
        inside[s:s + len(i)] = fetch(ijk) >= float(level)
    keys = _seed_keys(inside.view(P), pidx, probe, _brick_grid(shape))
    return _grow(fetch, keys, shape, org.tolist(), sp.tolist(), level, chunk, max_rounds, n, probe, what)


def sparse_volume_from_dense(volume, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """The SparseVolume of a CUDA float32 tensor [X, Y, Z] that is already there: the bricks sparse_volume(probe=1) selects, their values
    gathered from the tensor."""
    what = "sparse_volume_from_dense"
    require_cuda(volume)
    if volume.dim() != 3:
        raise ValueError(f"{what}: volume must be [X, Y, Z], got {tuple(volume.shape)}")
    vol = volume.detach().contiguous().float()
    shape = _shape3(vol.shape, what)
    hi = torch.tensor(shape, device=vol.device) - 1

    def fetch(ijk):
        i = torch.minimum(ijk, hi)                                             # entries past the lattice's end are never read
        return vol[i[:, 0], i[:, 1], i[:, 2]]

    pidx = [torch.arange(n, device=vol.device) for n in shape]
    keys = _seed_keys(vol >= float(level), pidx, 1, _brick_grid(shape))
    sp, org = _triple(spacing, "spacing"), _triple(origin, "origin")
    return _grow(fetch, keys, shape, list(org), list(sp), level, 2 ** 21, 1 << 30, vol.numel(), 1, what)


def marching_cubes_sparse(sv, level, normals=True, want_keys=False):
    """marching_cubes over the bricks of a SparseVolume (csrc/mesh_sparse.hip): -> (verts, faces, normals or None[, keys]) on the device,
    the mesh marching_cubes gives on the full lattice wherever the bricks cover the surface — the same bits; vertices ordered by (brick,
    point in the brick, axis), triangles by (brick, cell in the brick, table order).  keys [V] int64 = ((x * ny + y) * nz + z) * 3 + axis
    of every vertex: torch.argsort(keys) is the permutation into marching_cubes' order.  A brick through which the surface passes and
    that lacks a neighbour is open and raises ValueError (sparse_volume never returns one); the three counts are the only host read."""
    what = "marching_cubes_sparse"
    require_cuda(sv.values, sv.coords, sv.nbr)
    n, dev = sv.n_bricks, sv.values.device
    if tuple(sv.values.shape) != (n, _BRICK_POINTS) or tuple(sv.coords.shape) != (n, 3) or tuple(sv.nbr.shape) != (n, 27):
        raise ValueError(f"{what}: need values [n, 512], coords [n, 3] and nbr [n, 27], got {tuple(sv.values.shape)}, "
                         f"{tuple(sv.coords.shape)} and {tuple(sv.nbr.shape)}")
    values = sv.values.detach().contiguous().float()
    coords, nbr = sv.coords.contiguous().to(torch.int32), sv.nbr.contiguous().to(torch.int32)
    shape = _shape3(sv.shape, what)
    sp, org = _triple(sv.spacing, "spacing"), _triple(sv.origin, "origin")
    level = float(level)
    V = F = 0
    if n:
        ws, nbytes, counts, _ = _sparse_count(values, coords, nbr, shape, level, False)
        V, F, n_open = (int(c) & 0xffffffff for c in counts.cpu())             # the one host read
        if n_open:
            raise ValueError(f"{what}: {n_open} open bricks: the surface passes through them and a neighbour brick is missing")
        if V == 0xffffffff:
            raise ValueError(f"marching_cubes: the mesh of a {shape[0]}x{shape[1]}x{shape[2]} volume has more than 2^31 - 1 vertices or triangles")
    verts, nrm, faces, _ = _outputs(dev, V, F, normals, old_index=False)
    keys = torch.empty(V, dtype=torch.int64, device=dev) if want_keys else None
    if n:
        check(lib.cnerf_marching_cubes_sparse_emit(ptr(values), ptr(coords), ptr(nbr), n, *shape, level, org, sp, ptr(ws), nbytes, _p(verts),
                                                   _p(nrm), _p(faces), _p(keys), V, F, stream()), "marching_cubes_sparse_emit")
    return (verts, faces, nrm, keys) if want_keys else (verts, faces, nrm)


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


def components_workspace_bytes(V, F):
    return _bytes("mesh_components", int(V), int(F))


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
    ws, nbytes = _workspace(dev, "mesh_components", V, F)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    lg = 1 if largest else 0
    check(lib.cnerf_mesh_components_count(_p(f), V, F, mf, lg, ptr(ws), nbytes, ptr(counts), stream()), "mesh_components_count")
    V2, F2, _ = _read(counts, "remove_small_components", _BAD_INDEX)
    vo, no, fo, old = _outputs(dev, V2, F2, n is not None)
    check(lib.cnerf_mesh_components_emit(_p(v), _p(n), V, _p(f), F, mf, lg, ptr(ws), nbytes, _p(vo), _p(no), _p(fo), _p(old), V2, F2,
                                         stream()), "mesh_components_emit")
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
    return _bytes("mesh_cluster", int(V), int(F), (C.c_uint32 * 3)(*grid))


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
    ws, nbytes = _workspace(dev, "mesh_cluster", V, F, gg)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    check(lib.cnerf_mesh_cluster_count(_p(v), V, _p(f), F, og, cg, gg, ptr(ws), nbytes, ptr(counts), stream()), "mesh_cluster_count")
    K, F2, _ = _read(counts, "simplify", _BAD_INDEX)
    vo, no, fo, _ = _outputs(dev, K, F2, n is not None, old_index=False)
    check(lib.cnerf_mesh_cluster_emit(_p(v), _p(n), V, _p(f), F, og, cg, gg, ptr(ws), nbytes, _p(vo), _p(no), _p(fo), K, F2, stream()),
          "mesh_cluster_emit")
    return vo, fo, no


def decimate_workspace_bytes(V, F):
    return _bytes("mesh_decimate", int(V), int(F))


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
    ws, nbytes = _workspace(dev, "mesh_decimate", V, F)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    check(lib.cnerf_mesh_decimate_init(_p(v), V, _p(f), F, ptr(ws), nbytes, ptr(counts), stream()), "mesh_decimate_init")
    nv, nf, _, _ = _read(counts, "decimate", _DECIMATE_FLAGS)                   # one host read after init and after each round
    while nf > target:
        check(lib.cnerf_mesh_decimate_round(V, nf, target, ptr(ws), nbytes, ptr(counts), stream()), "mesh_decimate_round")
        nv, nf, done, _ = _read(counts, "decimate", _DECIMATE_FLAGS)
        if rounds is not None:
            rounds.append((nv, nf, done))
        if done == 0:
            break
    vo, no, fo, old = _outputs(dev, nv, nf, n is not None)
    check(lib.cnerf_mesh_decimate_emit(_p(n), V, nf, ptr(ws), nbytes, _p(vo), _p(no), _p(fo), _p(old), nv, nf, stream()), "mesh_decimate_emit")
    return vo, fo, no, old


def holes_workspace_bytes(V, F):
    return _bytes("mesh_holes", int(V), int(F))


_TOPOLOGY_COUNTS = ("vertices_used", "edges", "boundary_edges", "nonmanifold_edges", "pinched_vertices", "boundary_loops", "simple_loops",
                    "components", "degenerate_faces")


def topology(verts, faces):
    """What kind of surface a triangle mesh is, counted on the device (csrc/mesh_holes.hip; the rules are in include/customnerf_hip.h,
    cnerf_mesh_topology*).  Any triangle mesh (it need not be manifold): CUDA tensors verts [V, 3], faces [F, 3] (int).  -> dict of
    Python ints and bools from one host read, plus one device tensor:
    vertices_used (vertices in a face), faces, edges (distinct unordered vertex pairs; a face repeating an index adds no edge between the
    equal ones); boundary_edges (in one face), nonmanifold_edges (in more than two faces, or in two that use them in one direction);
    pinched_vertices (more than one boundary half-edge leaves them, or ends in them); boundary_loops (connected components of the graph
    of boundary edges) and simple_loops (those without a pinched vertex or an end of a non-manifold edge: the ones fill_holes closes);
    components (vertices joined by a face, labelled as by remove_small_components; vertices no face references are not counted);
    euler = vertices_used - edges + faces; degenerate_faces (faces repeating an index); watertight (at least one face and no boundary
    edge, non-manifold edge or degenerate face); loop_lengths [boundary_loops] int32 on the device, the edges of every loop in the order
    of the loops' labels (the smallest half-edge id 3 f + k on each).  A face index outside [0, V) raises ValueError."""
    v, f, _ = _mesh_args(verts, faces, None, "topology")
    V, F = v.shape[0], f.shape[0]
    dev = v.device
    r = [0] * len(_TOPOLOGY_COUNTS)
    if F:                                                                       # (no face: nothing to launch)
        ws, nbytes = _workspace(dev, "mesh_holes", V, F)
        counts = torch.empty(len(_TOPOLOGY_COUNTS) + 1, dtype=torch.int32, device=dev)
        check(lib.cnerf_mesh_topology(_p(f), V, F, ptr(ws), nbytes, ptr(counts), stream()), "mesh_topology")
        r = _read(counts, "topology", _BAD_INDEX)[:-1]                          # the one host read
    t = dict(zip(_TOPOLOGY_COUNTS, r))
    t["faces"] = F
    t["euler"] = t["vertices_used"] - t["edges"] + F
    t["watertight"] = F > 0 and not (t["boundary_edges"] or t["nonmanifold_edges"] or t["degenerate_faces"])
    t["loop_lengths"] = torch.empty(t["boundary_loops"], dtype=torch.int32, device=dev)
    if t["boundary_loops"]:
        check(lib.cnerf_mesh_topology_loops(V, F, ptr(ws), nbytes, ptr(t["loop_lengths"]), t["boundary_loops"], stream()), "mesh_topology_loops")
    return t


def _max_edges(max_edges, what):
    """max_edges of fill_holes as the entry points take it: 0 for None (no limit), else an int >= 3"""
    if max_edges is None:
        return 0
    if isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or not 3 <= max_edges < 2 ** 32:
        raise ValueError(f"{what}: max_edges must be None (no limit) or an int >= 3, got {max_edges!r}")
    return int(max_edges)


def fill_holes(verts, faces, normals=None, max_edges=None):
    """Close the boundary loops of a mesh on the device (csrc/mesh_holes.hip; the rules are in include/customnerf_hip.h,
    cnerf_mesh_holes_*).  The mesh must be edge-manifold and consistently oriented with no face repeating an index, as marching cubes,
    remove_small_components, decimate and TSDFVolume.extract give; anything else raises ValueError, as decimate does.  Every simple loop
    (topology()) of 3 <= n <= max_edges edges (None: no limit) is filled: a loop of 3 with the one face that reverses its half-edges, a
    longer one with a new vertex at the centroid of its vertices and a fan of n faces wound like the surface round it.  Loops through a
    pinched vertex and longer loops stay open and are counted.  A centroid fan across a large or non-planar hole is a coarse patch; the
    new vertex is an interior one, so smooth() moves it and decimate() may remove it.
    CUDA tensors verts [V, 3], faces [F, 3] (int), normals [V, 3] or None.  -> (verts [V', 3] float32, faces [F', 3] int32, normals
    [V', 3] or None, info).  The input vertices and faces (unreferenced vertices included) are the prefix of the output, bit for bit;
    new vertices follow in the order of the loops' labels, new faces in that order and, within a loop, in loop order from its label.
    The new vertex's normal is the normalised sum of its fan's face normals.  info: {'filled', 'skipped_pinched', 'skipped_long',
    'new_vertices', 'new_faces'}.  A mesh with nothing to fill comes back equal to the input."""
    me = _max_edges(max_edges, "fill_holes")
    v, f, n = _mesh_args(verts, faces, normals, "fill_holes")
    V, F = v.shape[0], f.shape[0]
    dev = v.device
    nv = nf = filled = pinched = long_ = 0
    if F:
        ws, nbytes = _workspace(dev, "mesh_holes", V, F)
        counts = torch.empty(6, dtype=torch.int32, device=dev)
        check(lib.cnerf_mesh_holes_count(_p(f), V, F, me, ptr(ws), nbytes, ptr(counts), stream()), "mesh_holes_count")
        nv, nf, filled, pinched, long_, _ = _read(counts, "fill_holes", _DECIMATE_FLAGS)          # the one host read
    info = {'filled': filled, 'skipped_pinched': pinched, 'skipped_long': long_, 'new_vertices': nv, 'new_faces': nf}
    if not F:
        return v.clone(), f.clone(), None if n is None else n.clone(), info
    vo, no, fo, _ = _outputs(dev, V + nv, F + nf, n is not None, old_index=False)
    check(lib.cnerf_mesh_holes_emit(_p(v), _p(n), V, _p(f), F, me, ptr(ws), nbytes, _p(vo), _p(no), _p(fo), V + nv, F + nf, stream()),
          "mesh_holes_emit")
    return vo, fo, no, info


def smooth_workspace_bytes(V, F):
    return _bytes("mesh_smooth", int(V), int(F))


def _smooth_init(v, f, what):
    """workspace of cnerf_mesh_smooth_* with the neighbour and face lists built, and its size"""
    V, F = v.shape[0], f.shape[0]
    ws, nbytes = _workspace(v.device, "mesh_smooth", V, F)
    flags = torch.empty(1, dtype=torch.int32, device=v.device)
    check(lib.cnerf_mesh_smooth_init(_p(f), V, F, ptr(ws), nbytes, ptr(flags), stream()), "mesh_smooth_init")
    _read(flags, what, _BAD_INDEX)
    return ws, nbytes


def _normals(v, f, n, ws, nbytes):
    V, F = v.shape[0], f.shape[0]
    no = torch.empty(V, 3, dtype=torch.float32, device=v.device)
    check(lib.cnerf_mesh_smooth_normals(_p(v), _p(n), V, _p(f), F, ptr(ws), nbytes, _p(no), stream()), "mesh_smooth_normals")
    return no


def smooth(verts, faces, iterations=10, lamb=0.5, mu=-0.53, normals=None, pin_boundary=True):
    """Taubin lambda|mu smoothing (Taubin 1995) with uniform weights on the device (csrc/mesh_smooth.hip; the rules are in
    include/customnerf_hip.h, cnerf_mesh_smooth_*): each iteration moves every vertex by lamb, then by mu (when mu != 0), times the offset
    from the mean of its neighbours (the distinct vertices sharing an edge with it).  The defaults are MeshLab's Taubin defaults; mu=0 is
    plain Laplacian smoothing, which shrinks the mesh.  With pin_boundary, vertices on an edge with one face keep their position bit for
    bit; a vertex no edge reaches never moves.  Any triangle mesh: CUDA tensors verts [V, 3], faces [F, 3] (int; need not be manifold),
    normals [V, 3] or None.  -> (verts [V, 3] float32, normals [V, 3] float32): the faces are unchanged and the normals are vertex_normals()
    of the smoothed positions (where a vertex's face normals sum to zero, its input normal, or zero without one).  Bad input raises
    ValueError."""
    v, f, n = _mesh_args(verts, faces, normals, "smooth")
    it = int(iterations)
    if it < 0 or it >= 2 ** 32:
        raise ValueError(f"smooth: iterations must be in [0, 2^32), got {iterations}")
    lamb, mu = float(lamb), float(mu)
    if not (math.isfinite(lamb) and 0.0 < lamb <= 1.0 and math.isfinite(mu) and -1.0 <= mu <= 0.0):
        raise ValueError(f"smooth: need 0 < lamb <= 1 and -1 <= mu <= 0, got lamb = {lamb}, mu = {mu}")
    V, F = v.shape[0], f.shape[0]
    ws, nbytes = _smooth_init(v, f, "smooth")
    vo = torch.empty(V, 3, dtype=torch.float32, device=v.device)
    check(lib.cnerf_mesh_smooth_steps(_p(v), V, F, it, lamb, mu, 1 if pin_boundary else 0, ptr(ws), nbytes, _p(vo), stream()),
          "mesh_smooth_steps")
    return vo, _normals(vo, f, n, ws, nbytes)


def vertex_normals(verts, faces, normals=None):
    """Area-weighted vertex normals on the device (csrc/mesh_smooth.hip): the normalised sum of (p1 - p0) x (p2 - p0) over the faces that hold
    the vertex, in increasing face index, in float32; where that sum is zero, the vertex's normal from `normals`, or zero without them.  CUDA
    tensors verts [V, 3], faces [F, 3] (int), normals [V, 3] or None.  -> normals [V, 3] float32.  Bad input raises ValueError."""
    v, f, n = _mesh_args(verts, faces, normals, "vertex_normals")
    ws, nbytes = _smooth_init(v, f, "vertex_normals")
    return _normals(v, f, n, ws, nbytes)


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



def atlas_layout(F, resolution):
    """(n, s) of the texture atlas of F faces on a resolution x resolution image: n cells per row, s texels per cell edge (the rules are in
    include/customnerf_hip.h, cnerf_mesh_atlas_*).  ValueError when the resolution is outside [16, 16384] or the cells would be smaller than
    4 x 4 texels."""
    F, R = int(F), int(resolution)
    if F < 0 or F >= 2 ** 31 or R < 16 or R > 16384:
        raise ValueError(f"atlas_layout: need 0 <= F < 2^31 and 16 <= resolution <= 16384, got F = {F}, resolution = {R}")
    n, s = C.c_uint32(0), C.c_uint32(0)
    if lib.cnerf_mesh_atlas_layout(F, R, C.byref(n), C.byref(s)) != 0:
        raise ValueError(f"atlas_layout: {F} faces leave cells of fewer than 4 x 4 texels on a {R} x {R} texture; decimate the mesh "
                         f"(target_faces=) or raise the resolution")
    return n.value, s.value


_NO_FIT = "decimate the mesh (target_faces=) or raise the resolution"
TEXTURE_LAYOUTS = ('uniform', 'area', 'projected')


class _BakeLayout:
    """A texture atlas layout as bake_texture uses it, built from the mesh (v, f, n of _mesh_args), the resolution R and `what`, the name its
    errors are raised under.  plan: the layout's public plan, if it has one; uvs [F, 3, 2]; flags [1], the device's index check; total,
    the cell texels.  fill(img, colour) writes the image texels no cell texel lies on, points(t0, t1, x, d) the points and directions of the
    cell texels [t0, t1), store(t0, t1, val, colour, img) their colours val [t1 - t0, >= 3] (colour: for a cell texel no face owns),
    tspace(t0, t1, tangents, m, out) the tangent-space codes out [t1 - t0, 3] of the object-space normals m [t1 - t0, >= 3] (None: the mesh's
    own normal at the texel) in the frames of tangents [F, 3, 4], for store."""
    plan = None

    def __init__(self, v, f, n, R):
        self.v, self.f, self.n, self.R, self.V, self.F = v, f, n, R, v.shape[0], f.shape[0]

    @staticmethod
    def precheck(F, R):
        """what bake_texture reports before it looks at its other arguments"""


class _UniformLayout(_BakeLayout):
    precheck = staticmethod(atlas_layout)

    def __init__(self, v, f, n, R, what, gutter=None):
        super().__init__(v, f, n, R)
        self.total = (self.F + 1) // 2 * atlas_layout(self.F, R)[1] ** 2
        self.uvs = torch.empty(self.F, 3, 2, dtype=torch.float32, device=v.device)
        self.flags = torch.empty(1, dtype=torch.int32, device=v.device)
        check(lib.cnerf_mesh_atlas_uvs(_p(f), self.V, self.F, R, _p(self.uvs), self.F, ptr(self.flags), stream()), "mesh_atlas_uvs")
        _read(self.flags, what, _BAD_INDEX)                                     # the one host read

    def fill(self, img, colour):
        check(lib.cnerf_mesh_atlas_fill(self.F, self.R, colour, ptr(img), stream()), "mesh_atlas_fill")

    def points(self, t0, t1, x, d):
        check(lib.cnerf_mesh_atlas_points(ptr(self.v), _p(self.n), self.V, ptr(self.f), self.F, self.R, t0, t1, ptr(self.flags), ptr(x), ptr(d),
                                          t1 - t0, stream()), "mesh_atlas_points")

    def tspace(self, t0, t1, tangents, m, out):
        check(lib.cnerf_mesh_atlas_tspace(ptr(self.v), _p(self.n), self.V, ptr(self.f), self.F, self.R, ptr(tangents), t0, t1, _p(m),
                                          m.stride(0) if m is not None else 0, ptr(self.flags), ptr(out), t1 - t0, stream()), "mesh_atlas_tspace")

    def store(self, t0, t1, val, colour, img):
        check(lib.cnerf_mesh_atlas_store(self.F, self.R, t0, t1, ptr(val), val.stride(0), colour, ptr(self.flags), ptr(img), stream()),
              "mesh_atlas_store")


class AtlasPlan:
    """The area-proportional atlas of a mesh (atlas_plan): resolution; e, the size-key threshold, and threshold, the edge length it stands
    for (faces whose longest edge is below it get the smallest cells, and every doubling above it doubles the cell edge); counts [K + 1],
    the faces per class (class k: cells of 4 * 2^k texels); cells [F, 4] int32 on the device, (X0, Y0, s, b) per face: its cell's origin
    texel and edge and whether it is the cell's face A (0) or B (1); texels, the number of cell texels, and tiles, the 4 x 4 tiles the
    cells cover (texels = 16 tiles <= resolution^2)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _AreaLayout(_BakeLayout):
    def __init__(self, v, f, n, R, what, gutter=None):
        super().__init__(v, f, n, R)
        V, F = self.V, self.F
        if R < 16 or R > 16384 or R & (R - 1):
            raise ValueError(f"{what}: the 'area' layout needs a resolution that is a power of two in [16, 16384], got {R}")
        no_fit = f"{what}: {F} faces leave cells of fewer than 4 x 4 texels on a {R} x {R} texture; {_NO_FIT}"
        if (F + 1) // 2 > (R // 4) ** 2:
            raise ValueError(no_fit)
        dev = v.device
        self.ws, self.nbytes = ws, nbytes = _workspace(dev, "mesh_atlas_sized", F)
        hist = torch.empty(2049, dtype=torch.int32, device=dev)
        check(lib.cnerf_mesh_atlas_sized_measure(_p(v), V, _p(f), F, ptr(ws), nbytes, ptr(hist), stream()), "mesh_atlas_sized_measure")
        h = (C.c_uint32 * 2048)(*_read(hist, what, _BAD_INDEX)[:2048])             # the one host read
        e, tiles, self.counts = C.c_uint32(0), C.c_uint32(0), (C.c_uint32 * 8)()
        if lib.cnerf_mesh_atlas_sized_layout(h, R, C.byref(e), self.counts, C.byref(tiles)) != 0:
            raise ValueError(no_fit)
        self.flags = hist[2048:]
        cells = torch.empty(F, 4, dtype=torch.int32, device=dev)
        check(lib.cnerf_mesh_atlas_sized_plan(F, R, e.value, self.counts, ptr(ws), nbytes, ptr(self.flags), _p(cells), F, stream()),
              "mesh_atlas_sized_plan")
        K = min(7, R.bit_length() - 3)
        thr = math.inf if e.value >= 2040 else math.sqrt(struct.unpack("<f", struct.pack("<I", e.value << 20))[0])
        self.plan = AtlasPlan(resolution=R, e=e.value, threshold=thr, counts=list(self.counts)[:K + 1], cells=cells, texels=16 * tiles.value,
                              tiles=tiles.value)
        self.total = self.plan.texels

    @cached_property
    def uvs(self):                                                              # computed when first asked for: atlas_plan does not ask
        uvs = torch.empty(self.F, 3, 2, dtype=torch.float32, device=self.v.device)
        check(lib.cnerf_mesh_atlas_sized_uvs(self.F, self.R, _p(self.plan.cells), ptr(self.flags), _p(uvs), self.F, stream()),
              "mesh_atlas_sized_uvs")
        return uvs

    def fill(self, img, colour):
        check(lib.cnerf_mesh_atlas_sized_fill(self.R, self.plan.tiles, colour, ptr(img), stream()), "mesh_atlas_sized_fill")

    def points(self, t0, t1, x, d):
        check(lib.cnerf_mesh_atlas_sized_points(ptr(self.v), _p(self.n), self.V, ptr(self.f), self.F, self.R, self.counts, ptr(self.ws),
                                                self.nbytes, t0, t1, ptr(self.flags), ptr(x), ptr(d), t1 - t0, stream()),
              "mesh_atlas_sized_points")

    def tspace(self, t0, t1, tangents, m, out):
        check(lib.cnerf_mesh_atlas_sized_tspace(ptr(self.v), _p(self.n), self.V, ptr(self.f), self.F, self.R, self.counts, ptr(self.ws),
                                                self.nbytes, ptr(tangents), t0, t1, _p(m), m.stride(0) if m is not None else 0,
                                                ptr(self.flags), ptr(out), t1 - t0, stream()), "mesh_atlas_sized_tspace")

    def store(self, t0, t1, val, colour, img):
        check(lib.cnerf_mesh_atlas_sized_store(self.F, self.R, self.counts, ptr(self.ws), self.nbytes, t0, t1, ptr(val), val.stride(0), colour,
                                               ptr(self.flags), ptr(img), stream()), "mesh_atlas_sized_store")


def atlas_plan(verts, faces, resolution):
    """The area-proportional texture atlas of a mesh on a resolution x resolution image (a power of two in [16, 16384]): every face gets a
    square cell of 4 * 2^k texels, k growing with its longest edge, so that texels per unit length vary by about a factor of two instead of
    with the face's size (the rules are in include/customnerf_hip.h, cnerf_mesh_atlas_sized_*).  CUDA tensors verts [V, 3], faces [F, 3]
    -> AtlasPlan.  ValueError on a face index outside [0, V), a resolution that is no power of two, or more faces than fit."""
    v, f, _ = _mesh_args(verts, faces, None, "atlas_plan")
    return _AreaLayout(v, f, None, int(resolution), "atlas_plan").plan


class ChartPlan:
    """The chart-based atlas of a mesh (chart_plan): resolution, gutter; charts, their number; density, texels per unit length; rects
    [C, 4] int32 on the device, (X0, Y0, w, h) of every chart's rectangle, gutter included; face_chart [F] int32 (-1: a face without area,
    which gets no texel) and face_class [F] int32 (2 axis + (the normal points down the axis), 6: none); owner [R, R] int32, the face
    every texel is baked from (-1: none); texels, the owned texels; overlap_texels, the (face, texel) pairs where a face covers a texel
    centre that another face owns (charts that fold over themselves in projection; 0 on a convex blob); coverage = texels / R^2."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _ProjectedLayout(_BakeLayout):
    def __init__(self, v, f, n, R, what, gutter=None):
        super().__init__(v, f, n, R)
        V, F = self.V, self.F
        g = int(gutter)
        if R < 16 or R > 16384:
            raise ValueError(f"{what}: the 'projected' layout needs a resolution in [16, 16384], got {R}")
        if g < 0 or g > 8:
            raise ValueError(f"{what}: gutter must be in [0, 8], got {gutter}")
        dev = v.device
        self.ws, self.nbytes = ws, nbytes = _workspace(dev, "mesh_atlas_proj", V, F, R)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        ext = torch.empty(F, 4, dtype=torch.float32, device=dev)
        fclass = torch.empty(F, dtype=torch.int32, device=dev)
        fchart = torch.empty(F, dtype=torch.int32, device=dev)
        check(lib.cnerf_mesh_atlas_proj_charts(_p(v), _p(n), V, _p(f), F, R, ptr(ws), nbytes, ptr(counts), _p(fclass), _p(fchart), F, _p(ext), F,
                                               stream()), "mesh_atlas_proj_charts")
        nc = _read(counts, what, _BAD_INDEX)[0]                                    # host read: C and the flags
        e = np.ascontiguousarray(ext[:nc].cpu().numpy())                           # host read: exactly the C extents
        rho = C.c_double(0.0)
        rects_h = np.zeros((nc, 4), np.int32)
        rc = lib.cnerf_mesh_atlas_proj_pack(e.ctypes.data_as(C.c_void_p), nc, R, g, C.byref(rho), rects_h.ctypes.data_as(C.c_void_p))
        if rc == -1:                                                               # CNERF_EINVAL with arguments in range: not even rho = 0 fits
            raise ValueError(f"{what}: {nc} charts with a gutter of {g} do not fit a {R} x {R} texture; {_NO_FIT}")
        check(rc, "mesh_atlas_proj_pack")
        rects = torch.from_numpy(rects_h).to(dev)
        self.uvs = torch.empty(F, 3, 2, dtype=torch.float32, device=dev)
        owner = torch.empty(R, R, dtype=torch.int32, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        self.flags = counts[1:]
        check(lib.cnerf_mesh_atlas_proj_raster(_p(v), V, _p(f), F, R, g, rho.value, _p(rects), nc, ptr(ws), nbytes, ptr(self.flags),
                                               _p(self.uvs), F, None, ptr(owner), ptr(totals), stream()), "mesh_atlas_proj_raster")
        self.total, overlap = (int(t) for t in totals.cpu())                       # host read: the totals
        self.plan = ChartPlan(resolution=R, gutter=g, charts=nc, density=rho.value, rects=rects, face_chart=fchart, face_class=fclass,
                              owner=owner, texels=self.total, overlap_texels=overlap, coverage=self.total / float(R * R))

    def fill(self, img, colour):
        check(lib.cnerf_mesh_atlas_proj_fill(self.V, self.F, self.R, ptr(self.ws), self.nbytes, colour, ptr(self.flags), ptr(img), stream()),
              "mesh_atlas_proj_fill")

    def points(self, t0, t1, x, d):
        check(lib.cnerf_mesh_atlas_proj_points(ptr(self.v), _p(self.n), self.V, ptr(self.f), self.F, self.R, ptr(self.ws), self.nbytes, t0, t1,
                                               ptr(self.flags), ptr(x), ptr(d), t1 - t0, stream()), "mesh_atlas_proj_points")

    def tspace(self, t0, t1, tangents, m, out):
        check(lib.cnerf_mesh_atlas_proj_tspace(ptr(self.v), _p(self.n), self.V, ptr(self.f), self.F, self.R, ptr(self.ws), self.nbytes,
                                               ptr(tangents), t0, t1, _p(m), m.stride(0) if m is not None else 0, ptr(self.flags), ptr(out),
                                               t1 - t0, stream()), "mesh_atlas_proj_tspace")

    def store(self, t0, t1, val, colour, img):                                  # every listed texel has an owner: no colour for the others
        check(lib.cnerf_mesh_atlas_proj_store(self.V, self.F, self.R, ptr(self.ws), self.nbytes, t0, t1, ptr(val), val.stride(0),
                                              ptr(self.flags), ptr(img), stream()), "mesh_atlas_proj_store")


_LAYOUTS = dict(zip(TEXTURE_LAYOUTS, (_UniformLayout, _AreaLayout, _ProjectedLayout)))


def chart_plan(verts, faces, resolution, normals=None, gutter=2):
    """The chart-based texture atlas of a mesh on a resolution x resolution image (16 to 16384, any value): faces are grouped into charts
    by the dominant axis of their normal (of the vertex normals' sum when `normals` is given and the face stays within 60 degrees of that
    axis), each chart is projected along its axis, the charts are packed at one texel density with `gutter` (0 to 8) texels grown round
    each (the rules are in include/customnerf_hip.h, cnerf_mesh_atlas_proj_*).  CUDA tensors verts [V, 3], faces [F, 3] -> ChartPlan.
    ValueError on a face index outside [0, V), a resolution or gutter out of range, or more charts than fit."""
    v, f, n = _mesh_args(verts, faces, normals, "chart_plan")
    return _ProjectedLayout(v, f, n, int(resolution), "chart_plan", gutter).plan


def bake_texture(verts, faces, resolution, color_fn, normals=None, chunk=2 ** 21, fill=(0, 0, 0), layout='uniform', source=None, reach=None,
                 normal_map=False, gutter=None):
    """Bake color_fn into a resolution x resolution RGB8 texture atlas of the mesh (csrc/mesh_texture.hip).  layout='uniform': each face pair
    owns a square cell of s x s texels (atlas_layout), whatever the faces' sizes; layout='area': a face's cell has 4 * 2^k texels per edge,
    k from its longest edge (atlas_plan; the resolution must be a power of two); layout='projected': the faces are grouped into charts by the
    axis of their normal, projected and packed at one density, with `gutter` texels (default 2) grown round every chart (chart_plan,
    csrc/mesh_charts.hip) — seams only between charts, a texture that reads as an image.  Every texel of a face is evaluated at the point of the
    face's plane under its centre, looking at the surface: color_fn(x [N, 3] float32, d [N, 3] float32) -> RGB in [0, 1], [N, >= 3], any
    float dtype, called on chunks of at most `chunk` texels.  d = -(interpolated vertex normal), or -(face normal) without normals.  Texels no face owns get `fill` (uint8 RGB).
    CUDA tensors verts [V, 3], faces [F, 3] (int), normals [V, 3] or None.  -> (uvs [F, 3, 2] float32: the UV of corner k of face f,
    v pointing up; texture [R, R, 3] uint8, row 0 at the top), on the device.  A face index outside [0, V) raises ValueError.
    source=bake_source(...) bakes from another mesh's surface, as mesh bakers do for a decimated mesh: every texel's point is projected
    onto the source along the mesh's normal within `reach` (project_to_surface(source, x, -d, reach); by default 2 % of the diagonal of
    the source's box — a documented default, not a measured optimum) and color_fn is asked at the projected point, looking against the
    source's normal there: color_fn(point, -normal).  A texel that finds no surface within reach keeps its own point and normal.
    normal_map=True also writes an object-space normal map [R, R, 3] uint8 with the same layout and store: 0.5 + 0.5 n of the source's
    normal at the projected point, or without a source of the mesh's own interpolated normal (-d); texels no face owns get
    (128, 128, 128).  normal_map='tangent' writes a tangent-space map instead, the kind glTF takes: the same normal in the frame (t, B, N)
    of its texel, N = -d, t and B from corner_tangents(verts, faces, uvs, normals) (the rule is in include/customnerf_hip.h,
    cnerf_mesh_tangent_*: red along +u, green along +v with v up); without a source every owned texel is (128, 128, 255), which is also
    the colour of the texels no face owns.  With source or normal_map the result is (uvs, texture, extra), extra = {'normal_map': the map or
    None, 'kinds': [4] int64 on the device, the cell texels handed to color_fn by the kind of their projection (project_to_surface; zeros
    without a source)} and, with a normal map, 'normal_space': 'object' or 'tangent' and for the latter 'tangents' [F, 3, 4] float32; with
    neither it is (uvs, texture) as above."""
    v, f, n = _mesh_args(verts, faces, normals, "bake_texture")
    if source is not None and not isinstance(source, BakeSource):
        raise ValueError("bake_texture: source must come from bake_source")
    if source is None and reach is not None:
        raise ValueError("bake_texture: reach needs a source")
    if source is not None and reach is None:
        reach = 0.02 * source.diagonal
        if not reach > 0.0:
            raise ValueError("bake_texture: the source has no valid face to take a default reach from")
    F, R = f.shape[0], int(resolution)
    if isinstance(normal_map, str) and normal_map != 'tangent':
        raise ValueError(f"bake_texture: normal_map must be False, True (object space) or 'tangent', got {normal_map!r}")
    tangent = isinstance(normal_map, str)
    if layout not in TEXTURE_LAYOUTS:
        raise ValueError(f"bake_texture: layout must be 'uniform', 'area' or 'projected', got {layout!r}")
    if gutter is not None and layout != 'projected':
        raise ValueError(f"bake_texture: gutter belongs to layout='projected', got layout={layout!r}")
    _LAYOUTS[layout].precheck(F, R)                                              # before fill and chunk: of two wrong arguments the uniform
                                                                                # layout has always reported the resolution first
    fl = tuple(int(c) for c in fill)
    if len(fl) != 3 or min(fl) < 0 or max(fl) > 255:
        raise ValueError(f"bake_texture: fill must be 3 values in [0, 255], got {fill}")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"bake_texture: chunk must be >= 1, got {chunk}")
    dev = v.device
    tex = torch.empty(R, R, 3, dtype=torch.uint8, device=dev)
    images = [(tex, (C.c_uint8 * 3)(*fl))]                                      # every image goes through the same fill and store
    if normal_map:
        images.append((torch.empty(R, R, 3, dtype=torch.uint8, device=dev), (C.c_uint8 * 3)(128, 128, 255 if tangent else 128)))
    kinds = torch.zeros(4, dtype=torch.int64, device=dev)
    # the layout last: it ends in a host read, and what is allocated after that read keeps the device waiting for the fill
    lay = _LAYOUTS[layout](v, f, n, R, "bake_texture", 2 if gutter is None else gutter)
    uvs, total = lay.uvs, lay.total
    for img, fc in images:
        lay.fill(img, fc)
    m = max(1, min(chunk, total))
    x = torch.empty(m, 3, dtype=torch.float32, device=dev)
    d = torch.empty(m, 3, dtype=torch.float32, device=dev)
    tangents = code = None
    if tangent:
        tangents = _tangents(v, f, uvs, n, "bake_texture")[0]
        code = torch.empty(m, 3, dtype=torch.float32, device=dev)
    for t0 in range(0, total, m):
        t1 = min(t0 + m, total)
        k = t1 - t0
        lay.points(t0, t1, x, d)
        if source is not None:
            pr = project_to_surface(source, x[:k], -d[:k], reach)
            look = -pr['normal']
            rgb = color_fn(pr['point'], look)
            kinds += (pr['kind'][:, None] == torch.arange(4, dtype=torch.uint8, device=dev)).sum(0)       # no host read
        else:
            look = d[:k]
            rgb = color_fn(x[:k], look)
        if not torch.is_tensor(rgb) or rgb.dim() != 2 or rgb.shape[0] != k or rgb.shape[1] < 3 or not rgb.is_floating_point():
            raise ValueError(f"bake_texture: color_fn must return a floating tensor [N, >= 3] for N = {k} points, got "
                             f"{tuple(rgb.shape) if torch.is_tensor(rgb) else type(rgb).__name__}")
        rgb = rgb.detach()[:, :3].float()
        if rgb.stride(1) != 1 or rgb.device != dev:
            rgb = rgb.to(dev).contiguous()
        if tangent:                                                             # without a source the encoded normal is the texel's own N
            lay.tspace(t0, t1, tangents, -look if source is not None else None, code)
        for (img, fc), val in zip(images, (rgb, code if tangent else look * -0.5 + 0.5 if normal_map else None)):
            lay.store(t0, t1, val, fc, img)
    if source is None and not normal_map:
        return uvs, tex
    extra = {'normal_map': images[1][0] if normal_map else None, 'kinds': kinds}
    if normal_map:
        extra['normal_space'] = 'tangent' if tangent else 'object'
    if tangent:
        extra['tangents'] = tangents
    return uvs, tex, extra


def tangent_workspace_bytes(V, F):
    return _bytes("mesh_tangent", int(V), int(F))


def _uv_args(f, uvs, what):
    require_cuda(uvs)
    if tuple(uvs.shape) != (f.shape[0], 3, 2):
        raise ValueError(f"{what}: uvs must be [F, 3, 2] for F = {f.shape[0]} faces, got {tuple(uvs.shape)}")
    return uvs.detach().contiguous().float()


def _weld(f, uv, V, what):
    """the weld pass -> (corner_vertex [F, 3], vertex_corner [W], the workspace and its size); the one host read: W and the flags"""
    F, dev = f.shape[0], f.device
    ws, nbytes = _workspace(dev, "mesh_tangent", V, F)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    cv = torch.empty(F, 3, dtype=torch.int32, device=dev)
    vc = torch.empty(3 * F, dtype=torch.int32, device=dev)
    check(lib.cnerf_mesh_tangent_weld(_p(f), _p(uv), V, F, ptr(ws), nbytes, ptr(counts), _p(cv), F, _p(vc), 3 * F, stream()),
          "mesh_tangent_weld")
    W, _ = _read(counts, what, _BAD_INDEX)
    return cv, vc[:W], ws, nbytes


def _tangents(v, f, uv, n, what):
    """weld, then frames -> (tangents [F, 3, 4], corner_vertex, vertex_corner, the workspace and its size)"""
    V, F = v.shape[0], f.shape[0]
    cv, vc, ws, nbytes = _weld(f, uv, V, what)
    tan = torch.empty(F, 3, 4, dtype=torch.float32, device=v.device)
    check(lib.cnerf_mesh_tangent_frames(_p(v), _p(f), _p(uv), _p(n), V, F, ptr(ws), nbytes, _p(tan), F, stream()), "mesh_tangent_frames")
    return tan, cv, vc, ws, nbytes


def weld_corners(faces, uvs, V=None):
    """Weld the face corners of a UV-mapped mesh into vertices, on the device (csrc/mesh_tangent.hip; the rules are in
    include/customnerf_hip.h, cnerf_mesh_tangent_*): corners with the same vertex index and the same UV (bit for bit) are one output vertex;
    a vertex on a seam becomes one per chart.  Output vertices are numbered by ascending vertex index, within a vertex by their smallest
    corner (corner c = 3 f + k).  CUDA tensors faces [F, 3] (int), uvs [F, 3, 2] float32; V: the number of vertices the faces index
    (default: the largest index + 1).  -> (corner_vertex [F, 3] int32, vertex_corner [W] int32: the smallest corner of every output
    vertex).  A face index outside [0, V) raises ValueError."""
    require_cuda(faces)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"weld_corners: faces must be [F, 3], got {tuple(faces.shape)}")
    f = faces.detach().contiguous().to(torch.int32)
    uv = _uv_args(f, uvs, "weld_corners")
    if V is None:
        V = int(f.max()) + 1 if f.numel() else 0
    V = int(V)
    if V < 0:
        raise ValueError("weld_corners: a face index lies outside [0, V)")
    return _weld(f, uv, V, "weld_corners")[:2]


def corner_tangents(verts, faces, uvs, normals=None):
    """Tangent frames of a UV-mapped mesh, one per face corner, on the device (csrc/mesh_tangent.hip; the rules are in
    include/customnerf_hip.h): the corners weld_corners joins share one frame, the area-weighted sum of their faces' unit tangents
    (the direction of +u on the surface), made orthogonal to the vertex normal (without `normals`: to the area-weighted face normal of
    the group) and normalised, computed in float64 in a fixed order; w = +1 or -1 says whether the bitangent w (n x t) follows +v (v up).
    Faces without UV area or without area give nothing; a vertex left without a tangent takes the axis most orthogonal to its normal.
    CUDA tensors verts [V, 3], faces [F, 3] (int), uvs [F, 3, 2], normals [V, 3] or None -> tangents [F, 3, 4] float32 (x, y, z, w).
    A face index outside [0, V) raises ValueError."""
    v, f, n = _mesh_args(verts, faces, normals, "corner_tangents")
    return _tangents(v, f, _uv_args(f, uvs, "corner_tangents"), n, "corner_tangents")[0]


def gltf_vertices(verts, faces, uvs, normals=None):
    """The vertex and index buffers of a glTF primitive for a UV-mapped mesh, on the device: weld_corners, corner_tangents, then a
    gather.  -> dict: positions [W, 3], normals [W, 3] (the vertex normals as given, or without them the unit normal each frame was built
    on), uvs [W, 2] stored as (u, 1 - v) (glTF's v points down), tangents [W, 4] float32 and indices [F, 3] uint32 (= corner_vertex),
    for write_glb.  One host read (W and the index check)."""
    v, f, n = _mesh_args(verts, faces, normals, "gltf_vertices")
    uv = _uv_args(f, uvs, "gltf_vertices")
    V, F, dev = v.shape[0], f.shape[0], v.device
    tan, cv, vc, ws, nbytes = _tangents(v, f, uv, n, "gltf_vertices")
    W = vc.shape[0]
    out = {'positions': torch.empty(W, 3, dtype=torch.float32, device=dev), 'normals': torch.empty(W, 3, dtype=torch.float32, device=dev),
           'uvs': torch.empty(W, 2, dtype=torch.float32, device=dev), 'tangents': torch.empty(W, 4, dtype=torch.float32, device=dev)}
    idx = torch.empty(F, 3, dtype=torch.int32, device=dev)                      # the kernel writes uint32 < 2^31: the same bits
    check(lib.cnerf_mesh_tangent_vertices(_p(v), _p(f), _p(uv), _p(n), _p(tan), _p(cv), _p(vc), V, F, W, ptr(ws), nbytes, _p(out['positions']),
                                          _p(out['normals']), _p(out['uvs']), _p(out['tangents']), _p(idx), stream()), "mesh_tangent_vertices")
    out['indices'] = idx.view(torch.uint32) if hasattr(torch, 'uint32') else idx
    return out


_CONVENTIONS = {'nerfstudio': 0, 'ngp': 1}
_CULL = {'none': 0, 'back': 1, 'front': 2}
_SHADING = {'colors': 0, 'texture': 1, 'normals': 2, 'depth': 3}


def raster_workspace_bytes(V, F, H, W):
    return _bytes("mesh_raster", int(V), int(F), int(H), int(W))


def _camera(c2w, intrinsics, H, W, what):
    """(c2w as 12 host floats, fx, fy, cx, cy, H, W) of one pinhole camera"""
    m = _host(c2w, np.float32)
    if m.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"{what}: c2w must be [3, 4] or [4, 4], got {m.shape}")
    k = tuple(float(x) for x in intrinsics)
    if len(k) != 4:
        raise ValueError(f"{what}: intrinsics must be (fx, fy, cx, cy), got {len(k)} values")
    H, W = int(H), int(W)
    if H < 0 or W < 0 or H * W >= 2 ** 31:
        raise ValueError(f"{what}: need H, W >= 0 and H * W < 2^31, got H = {H}, W = {W}")
    return (C.c_float * 12)(*m[:3].ravel().tolist()), k, H, W


def _cameras(c2w, N, intrinsics, H, W, what, per="image"):
    """(c2w [N, 3|4, 4] as a host array, the N cameras' 12 floats each, (fx, fy, cx, cy), H, W) of N pinhole views with one set of
    intrinsics; a single [3|4, 4] c2w is one view"""
    m = _host(c2w, np.float32)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[0] != N:
        raise ValueError(f"{what}: need one c2w per {per}, got {m.shape} for {N} views")
    _, k, H, W = _camera(np.zeros((3, 4), np.float32), intrinsics, H, W, what)
    return m, [_camera(m[v], intrinsics, H, W, what)[0] for v in range(N)], k, H, W


def rasterize(verts, faces, c2w, intrinsics, H, W, convention='nerfstudio', near=0.01, cull='none'):
    """Visibility buffer of a triangle mesh seen through one pinhole camera, on the device (csrc/mesh_raster.hip; the rules are in
    include/customnerf_hip.h, cnerf_mesh_raster_*).  The camera is generate_rays': c2w [3, 4] or [4, 4] (tensor or array), intrinsics
    (fx, fy, cx, cy), convention 'nerfstudio' or 'ngp'; pixels are sampled at their centres.  cull: 'none', 'back' or 'front' (faces wound
    outwards, as marching cubes emits them, are front-facing from outside).  A face with a vertex nearer than `near` along the camera axis,
    or behind the camera, is dropped whole (no clipping).  CUDA tensors verts [V, 3], faces [F, 3] (int).
    -> dict of device tensors face [H, W] int32 (-1: none), depth [H, W] float32 (camera-axis depth, +inf: none), bary [H, W, 3] float32
    (perspective-correct, in the face's vertex order), and dropped: the number of dropped faces.  Bad input raises ValueError."""
    v, f, _ = _mesh_args(verts, faces, None, "rasterize")
    m, k, H, W = _camera(c2w, intrinsics, H, W, "rasterize")
    if convention not in _CONVENTIONS:
        raise ValueError(f"rasterize: convention must be 'nerfstudio' or 'ngp', got {convention!r}")
    if cull not in _CULL:
        raise ValueError(f"rasterize: cull must be 'none', 'back' or 'front', got {cull!r}")
    near = float(near)
    if not (math.isfinite(near) and all(math.isfinite(x) for x in k) and k[0] != 0.0 and k[1] != 0.0):
        raise ValueError(f"rasterize: need finite intrinsics with fx, fy != 0 and a finite near, got {k}, near = {near}")
    V, F = v.shape[0], f.shape[0]
    dev = v.device
    ws, nbytes = _workspace(dev, "mesh_raster", V, F, H, W)
    face = torch.empty(H, W, dtype=torch.int32, device=dev)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    bary = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    check(lib.cnerf_mesh_raster_visibility(_p(v), V, _p(f), F, m, *k, H, W, _CONVENTIONS[convention], near, _CULL[cull], ptr(ws), nbytes,
                                           _p(face), _p(depth), _p(bary), ptr(counts), stream()), "mesh_raster_visibility")
    dropped, _ = _read(counts, "rasterize", _BAD_INDEX)                        # the one host read
    return {'face': face, 'depth': depth, 'bary': bary, 'dropped': dropped}


def render_mesh(verts, faces, c2w, intrinsics, H, W, *, colors=None, uvs=None, texture=None, normals=None, shading=None, bg=(0, 0, 0),
                depth_range=None, **raster_kw):
    """Shaded preview of a triangle mesh from one camera, on the device: rasterize(verts, faces, c2w, intrinsics, H, W, **raster_kw), then
    one shading pass.  shading: 'texture' (uvs [F, 3, 2] float32 and texture [R, R, 3] uint8 as bake_texture returns them: bilinear, v up,
    clamped to the edge), 'colors' (colors [V, 3] uint8, interpolated), 'normals' (0.5 + 0.5 n of the interpolated unit normal; without
    `normals` these are vertex_normals() of the mesh) or 'depth' (grey, (depth - d0) / (d1 - d0) for depth_range = (d0, d1), by default
    the smallest and largest hit depth).  shading=None picks texture when uvs and texture are given, else colours, else normals.  Pixels no
    face covers get `bg` (uint8 RGB).  -> (image [H, W, 3] uint8, mask [H, W] bool, the dict of rasterize), on the device.  Inconsistent
    arguments raise ValueError."""
    v, f, n = _mesh_args(verts, faces, normals, "render_mesh")
    V, F = v.shape[0], f.shape[0]
    if shading is None:
        shading = 'texture' if uvs is not None and texture is not None else 'colors' if colors is not None else 'normals'
    if shading not in _SHADING:
        raise ValueError(f"render_mesh: shading must be one of {sorted(_SHADING)} or None, got {shading!r}")
    b = tuple(int(c) for c in bg)
    if len(b) != 3 or min(b) < 0 or max(b) > 255:
        raise ValueError(f"render_mesh: bg must be 3 values in [0, 255], got {bg}")
    dev = v.device
    col = uv = tex = None
    R, d0, d1 = 0, 0.0, 1.0
    if shading == 'colors':
        if colors is None or tuple(colors.shape) != (V, 3) or colors.dtype != torch.uint8:
            raise ValueError(f"render_mesh: shading='colors' needs colors [V, 3] uint8 for V = {V}, got "
                             f"{None if colors is None else (tuple(colors.shape), colors.dtype)}")
        require_cuda(colors)
        col = colors.detach().contiguous()
    elif shading == 'texture':
        if uvs is None or texture is None:
            raise ValueError("render_mesh: shading='texture' needs uvs and texture")
        require_cuda(uvs, texture)
        if tuple(uvs.shape) != (F, 3, 2):
            raise ValueError(f"render_mesh: uvs must be [F, 3, 2] for F = {F} faces, got {tuple(uvs.shape)}")
        if texture.dim() != 3 or texture.shape[0] != texture.shape[1] or texture.shape[2] != 3 or texture.dtype != torch.uint8 or \
                not 1 <= texture.shape[0] <= 16384:
            raise ValueError(f"render_mesh: texture must be [R, R, 3] uint8 with 1 <= R <= 16384, got {tuple(texture.shape)} {texture.dtype}")
        uv, tex, R = uvs.detach().contiguous().float(), texture.detach().contiguous(), texture.shape[0]
    elif shading == 'depth' and depth_range is not None:
        d0, d1 = (float(x) for x in depth_range)
        if not (math.isfinite(d0) and math.isfinite(d1)):
            raise ValueError(f"render_mesh: depth_range must be two finite values, got {depth_range}")
    vis = rasterize(v, f, c2w, intrinsics, H, W, **raster_kw)
    H, W = vis['face'].shape
    if shading == 'normals' and n is None:
        n = vertex_normals(v, f)
    if shading == 'depth' and depth_range is None:
        hit = vis['depth'][vis['face'] >= 0]
        if hit.numel():
            d0, d1 = (float(x) for x in torch.aminmax(hit))
    image = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
    check(lib.cnerf_mesh_raster_shade(_p(vis['face']), _p(vis['depth']), _p(vis['bary']), H, W, _p(f), V, F, _SHADING[shading], _p(col), _p(uv),
                                      _p(tex), R, _p(v), _p(n), d0, d1, (C.c_uint8 * 3)(*b), _p(image), _p(mask), stream()),
          "mesh_raster_shade")
    return image, mask != 0, vis


# ------------------------------------------------------------------------------------------------ TSDF fusion of depth maps
_DEPTH_KINDS = {'z': 0, 'ray': 1}


class TSDFVolume:
    """Depth maps fused into a truncated signed distance volume on marching cubes' lattice, on the device (csrc/mesh_tsdf.hip; the rules
    are in include/customnerf_hip.h, cnerf_tsdf_*): the zero level is the surface the views show, with no density threshold to tune.
    shape (nx, ny, nz) >= 2 each and at most 2^31 - 1 points, origin / spacing 3 floats as marching_cubes takes them, trunc > 0 the
    truncation distance in world units (a few lattice steps: below about 3 the observed band round the surface has holes).  The state
    [n, 2] float32 = (sum of w s, sum of w) per point, s positive inside, lives on `device` (default: that of the first depth map) and is
    allocated by the first integrate.  `views` counts the integrated views."""

    def __init__(self, shape, origin, spacing, trunc, device=None):
        self.shape = _shape3(shape, "TSDFVolume")
        if math.prod(self.shape) >= 2 ** 31:
            raise ValueError(f"TSDFVolume: a lattice of {self.shape} has 2^31 points or more")
        self._org, self._sp = _triple(origin, "origin"), _triple(spacing, "spacing")
        self.origin, self.spacing = tuple(self._org), tuple(self._sp)
        self.trunc = float(trunc)
        if not (math.isfinite(self.trunc) and self.trunc > 0.0):
            raise ValueError(f"TSDFVolume: trunc must be finite and > 0, got {trunc}")
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != 'cuda':
            raise RuntimeError("customnerf_amd: tensors must live on the GPU (HIP device memory); there is no CPU path")
        self.views = 0
        self._state = None
        self._seen = None                                                       # (views, fill) -> (volume, observed points) of the last finalize

    @property
    def state(self):
        """[n, 2] float32 on the device: (acc, weight) per lattice point, z fastest"""
        if self._state is None:
            self._state = torch.zeros(math.prod(self.shape), 2, dtype=torch.float32, device=self.device or torch.device('cuda'))
            self.device = self._state.device
        return self._state

    def integrate(self, depth, c2w, intrinsics, convention='nerfstudio', depth_kind='ray', weights=None, near=0.01):
        """Fuse N views: depth [N, H, W] or [H, W] float32 CUDA ('ray': metric distance along the pixel's ray, what a renderer returns;
        'z': camera-axis depth, what rasterize returns; +inf: the ray hit nothing, free space all the way; NaN, 0 or negative: the pixel
        says nothing), c2w [N, 3|4, 4] or one [3|4, 4] (tensor or array), intrinsics (fx, fy, cx, cy) and convention as generate_rays and
        rasterize take them, weights None or like depth (a pixel with weight 0 says nothing).  Points nearer than `near` along the camera
        axis are not touched.  The views are summed in index order: any split into calls gives the same state.  -> self."""
        require_cuda(depth, weights)
        if depth.dim() == 2:
            depth = depth[None]
        if depth.dim() != 3:
            raise ValueError(f"TSDFVolume.integrate: depth must be [N, H, W] or [H, W], got {tuple(depth.shape)}")
        N, H, W = depth.shape
        if weights is not None:
            if weights.dim() == 2:
                weights = weights[None]
            if tuple(weights.shape) != (N, H, W):
                raise ValueError(f"TSDFVolume.integrate: weights must be shaped like depth, got {tuple(weights.shape)} and {(N, H, W)}")
        _, views, k, H, W = _cameras(c2w, N, intrinsics, H, W, "TSDFVolume.integrate", per="depth map")
        cams = (C.c_float * (12 * max(N, 1)))()
        for v in range(N):
            cams[12 * v:12 * v + 12] = list(views[v])
        if convention not in _CONVENTIONS:
            raise ValueError(f"TSDFVolume.integrate: convention must be 'nerfstudio' or 'ngp', got {convention!r}")
        if depth_kind not in _DEPTH_KINDS:
            raise ValueError(f"TSDFVolume.integrate: depth_kind must be 'ray' or 'z', got {depth_kind!r}")
        near = float(near)
        if not (math.isfinite(near) and all(math.isfinite(x) for x in k) and k[0] != 0.0 and k[1] != 0.0):
            raise ValueError(f"TSDFVolume.integrate: need finite intrinsics with fx, fy != 0 and a finite near, got {k}, near = {near}")
        if self.device is not None and depth.device != self.device:
            raise ValueError(f"TSDFVolume.integrate: the volume lives on {self.device}, depth on {depth.device}")
        self.device = depth.device
        d = depth.detach().contiguous().float()
        w = None if weights is None else weights.detach().contiguous().float()
        check(lib.cnerf_tsdf_integrate(ptr(self.state), *self.shape, self._org, self._sp, self.trunc, _p(d), _p(w), N, H, W, cams, *k,
                                       _CONVENTIONS[convention], near, _DEPTH_KINDS[depth_kind], stream()), "tsdf_integrate")
        self.views += N
        return self

    def _finalize(self, fill):
        fill = float(fill)
        if self._seen is None or self._seen[0] != (self.views, fill):
            vol = torch.empty(self.shape, dtype=torch.float32, device=self.state.device)
            count = torch.empty(1, dtype=torch.int32, device=vol.device)
            check(lib.cnerf_tsdf_finalize(ptr(self.state), *self.shape, fill, ptr(vol), ptr(count), stream()), "tsdf_finalize")
            self._seen = ((self.views, fill), vol, int(count.item()) & 0xffffffff)
        return self._seen[1], self._seen[2]

    def volume(self, fill=-1.0):
        """[nx, ny, nz] float32: acc / weight where a view said something, `fill` elsewhere (-1: free space); positive inside"""
        return self._finalize(fill)[0]

    @property
    def observed(self):
        """share of the lattice points with weight > 0"""
        return self._finalize(-1.0)[1] / math.prod(self.shape)

    def face_keep(self, verts, faces):
        """[F] bool: the lattice cell that holds the face's centroid has eight observed corners"""
        v, f, _ = _mesh_args(verts, faces, None, "TSDFVolume.face_keep")
        keep = torch.empty(f.shape[0], dtype=torch.uint8, device=f.device)
        check(lib.cnerf_tsdf_face_keep(ptr(self.state), *self.shape, self._org, self._sp, _p(v), v.shape[0], _p(f), f.shape[0], _p(keep),
                                       stream()), "tsdf_face_keep")
        return keep != 0

    def extract(self, fill=-1.0):
        """The fused surface: marching_cubes(volume(fill), 0.0) without its gradient normals (they would read `fill` next to unobserved
        points), minus the faces whose cell has an unobserved corner — the shell where "behind the surface" meets "never observed" — and
        the vertices only they used; face order is kept.  -> (verts [V, 3] float32, faces [F, 3] int32 wound outwards, normals [V, 3]
        float32: vertex_normals of the result, info {'observed': share of observed points, 'dropped_faces'})."""
        vol, seen = self._finalize(fill)
        verts, faces, _ = marching_cubes(vol, 0.0, spacing=self.spacing, origin=self.origin, normals=False)
        keep = self.face_keep(verts, faces)
        kept = faces[keep]
        used = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
        used[kept.reshape(-1).long()] = True
        new_index = (torch.cumsum(used, 0) - 1).to(torch.int32)
        verts, faces = verts[used].contiguous(), new_index[kept.long()].contiguous()
        info = {'observed': seen / math.prod(self.shape), 'dropped_faces': int(keep.numel() - kept.shape[0])}
        return verts, faces, vertex_normals(verts, faces), info


# ------------------------------------------------------------------------------------------------ colour fused from rendered views
_VIEW_BATCH = 16                                                                # views per launch of cnerf_view_colors_accumulate


class ViewColors:
    """Colour of surface points blended from the rendered views that see them, on the device (csrc/mesh_view_colors.hip; the rules are
    in include/customnerf_hip.h, cnerf_view_colors_*): a bake_texture color_fn that returns what the renders show — the composited
    colour along camera rays — in place of one point query of the field.  images [N, H, W, 3] float32 CUDA, depth [N, H, W] float32
    CUDA: the depth of THE SURFACE THE QUERIED POINTS LIE ON from each camera (rasterize(...)['depth'] of that mesh with depth_kind='z';
    'ray' takes a distance along the ray), never a NeRF's own depth; c2w [N, 3|4, 4] (tensor or array), intrinsics (fx, fy, cx, cy)
    and convention as generate_rays and rasterize take them; weights None or like depth (a rendered opacity: a pixel with weight 0 says
    nothing).  A view sees a point when the point lies at least `near` in front of it, the 2 x 2 pixels round its projection lie in
    the image and all four depths are finite and within depth_tol of the point's — required: a geometric scale only the caller knows,
    a few times the pixel footprint on the surface — and the cosine between the normal and the direction to the camera exceeds
    min_cos; its bilinear colour enters with weight cos^power times the bilinear pixel weight.  power (an integer 1..8) and min_cos
    (in [0, 1)) are documented defaults, not measured optima.  Pinhole views only, and no exposure compensation between views.
    vc(x [M, 3], d [M, 3]) -> [M, 3] float32 is the color_fn: the normal is -d.  Where no view saw the point the row comes from
    `fallback`, another color_fn evaluated for the whole chunk (no host read), else it is `fill` (3 floats).  vc.counts [3] int64 on the
    device adds up, over the calls, the points seen by 0, 1 and >= 2 views; reset_counts() clears it.  The views are summed in index
    order with no atomics: the result does not depend on how they are cut into launches.  Bad arguments raise ValueError before any
    launch."""

    def __init__(self, images, depth, c2w, intrinsics, depth_tol, convention='nerfstudio', depth_kind='z', weights=None, power=2, min_cos=0.2,
                 near=0.01, fallback=None, fill=(0, 0, 0)):
        if images.dim() != 4 or images.shape[3] != 3:
            raise ValueError(f"ViewColors: images must be [N, H, W, 3], got {tuple(images.shape)}")
        N, H, W = images.shape[:3]
        if tuple(depth.shape) != (N, H, W):
            raise ValueError(f"ViewColors: depth must be [N, H, W] like images, got {tuple(depth.shape)} and {(N, H, W)}")
        if weights is not None and tuple(weights.shape) != (N, H, W):
            raise ValueError(f"ViewColors: weights must be shaped like depth, got {tuple(weights.shape)} and {(N, H, W)}")
        for name, t in (("images", images), ("depth", depth), ("weights", weights)):
            if t is not None and t.dtype != torch.float32:
                raise ValueError(f"ViewColors: {name} must be float32, got {t.dtype}")
            if t is not None and t.device != images.device:
                raise ValueError(f"ViewColors: {name} lives on {t.device}, images on {images.device}")
        m, self._cams, k, H, W = _cameras(c2w, N, intrinsics, H, W, "ViewColors")
        if not np.isfinite(m[:, :3]).all():
            raise ValueError("ViewColors: c2w holds non-finite values")
        if convention not in _CONVENTIONS:
            raise ValueError(f"ViewColors: convention must be 'nerfstudio' or 'ngp', got {convention!r}")
        if depth_kind not in _DEPTH_KINDS:
            raise ValueError(f"ViewColors: depth_kind must be 'ray' or 'z', got {depth_kind!r}")
        near = float(near)
        if not (math.isfinite(near) and all(math.isfinite(x) for x in k) and k[0] != 0.0 and k[1] != 0.0):
            raise ValueError(f"ViewColors: need finite intrinsics with fx, fy != 0 and a finite near, got {k}, near = {near}")
        self.depth_tol = float(depth_tol)
        if not (math.isfinite(self.depth_tol) and self.depth_tol > 0.0):
            raise ValueError(f"ViewColors: depth_tol must be finite and > 0, got {depth_tol}")
        if isinstance(power, bool) or not isinstance(power, (int, np.integer)) or not 1 <= power <= 8:
            raise ValueError(f"ViewColors: power must be an integer in 1..8, got {power!r}")
        self.min_cos = float(min_cos)
        if not 0.0 <= self.min_cos < 1.0:
            raise ValueError(f"ViewColors: min_cos must lie in [0, 1), got {min_cos}")
        if fallback is not None and not callable(fallback):
            raise ValueError(f"ViewColors: fallback must be None or a color_fn(x, d), got {type(fallback).__name__}")
        fl = tuple(float(c) for c in fill)
        if len(fl) != 3 or not all(math.isfinite(c) for c in fl):
            raise ValueError(f"ViewColors: fill must be 3 finite values, got {fill}")
        require_cuda(images, depth, weights)                                    # last: everything above is checked without a device
        self.images, self.depth = images.detach().contiguous(), depth.detach().contiguous()
        self.weights = None if weights is None else weights.detach().contiguous()
        self.views, self.H, self.W, self.device = N, H, W, images.device
        self.intrinsics, self.near, self.power = k, near, int(power)
        self.convention, self.depth_kind = convention, depth_kind
        self.fallback, self._fill = fallback, (C.c_float * 3)(*fl)
        self.counts = torch.zeros(3, dtype=torch.int64, device=self.device)

    def reset_counts(self):
        self.counts.zero_()

    def _points(self, x, normals, what):
        require_cuda(x, normals)
        if x.dim() != 2 or x.shape[1] != 3 or tuple(normals.shape) != tuple(x.shape):
            raise ValueError(f"{what}: points and normals must both be [M, 3], got {tuple(x.shape)} and {tuple(normals.shape)}")
        if x.shape[0] >= 2 ** 31:
            raise ValueError(f"{what}: at most 2^31 - 1 points a call, got {x.shape[0]}")
        if x.device != self.device or normals.device != self.device:
            raise ValueError(f"{what}: the views live on {self.device}, the points on {x.device}")
        return x.detach().contiguous().float(), normals.detach().contiguous().float()

    def accumulate(self, x, normals, state=None, seen=None, views=None):
        """Add the views `views` (a slice of the view indices; default all) to the sums of the points x [M, 3] with unit normals [M, 3]:
        state [M, 4] float32 (sum of w r, w g, w b, w) and seen [M] int32 (the views that added), both zero when not given, updated in
        place, one launch per 16 views.  -> (state, seen)"""
        x, n = self._points(x, normals, "ViewColors.accumulate")
        M = x.shape[0]
        if state is None:
            state = torch.zeros(M, 4, dtype=torch.float32, device=self.device)
        if seen is None:
            seen = torch.zeros(M, dtype=torch.int32, device=self.device)
        if tuple(state.shape) != (M, 4) or state.dtype != torch.float32 or tuple(seen.shape) != (M,) or seen.dtype != torch.int32 or \
                not state.is_contiguous() or not seen.is_contiguous() or state.device != self.device or seen.device != self.device:
            raise ValueError(f"ViewColors.accumulate: state must be contiguous [M, 4] float32 and seen [M] int32 for M = {M} on {self.device}")
        idx = range(self.views)[slice(None) if views is None else views]
        if not isinstance(idx, range) or (len(idx) and idx.step != 1):
            raise ValueError(f"ViewColors.accumulate: views must be a slice of consecutive views, got {views!r}")
        for b in range(idx.start, idx.start + len(idx), _VIEW_BATCH):
            nb = min(_VIEW_BATCH, idx.start + len(idx) - b)
            cams = (C.c_float * (12 * nb))()
            for v in range(nb):
                cams[12 * v:12 * v + 12] = list(self._cams[b + v])
            check(lib.cnerf_view_colors_accumulate(_p(x), _p(n), M, _p(self.images[b:b + nb]), _p(self.depth[b:b + nb]),
                                                   None if self.weights is None else _p(self.weights[b:b + nb]), nb, self.H, self.W, cams,
                                                   *self.intrinsics, _CONVENTIONS[self.convention], self.near, _DEPTH_KINDS[self.depth_kind],
                                                   self.depth_tol, self.min_cos, self.power, _p(state), _p(seen), stream()),
                  "view_colors_accumulate")
        return state, seen

    def resolve(self, state, seen, fallback=None):
        """[M, 3] float32: acc / weight where a view saw the point, else the row of `fallback` ([M, 3] float32 tensor or None), else
        `fill`; the points seen by 0, 1 and >= 2 views are added to `counts`."""
        M = state.shape[0]
        if fallback is not None and (tuple(fallback.shape) != (M, 3) or fallback.dtype != torch.float32 or not fallback.is_contiguous() or
                                     fallback.device != self.device):
            raise ValueError(f"ViewColors.resolve: fallback must be contiguous [M, 3] float32 for M = {M} on {self.device}")
        out = torch.empty(M, 3, dtype=torch.float32, device=self.device)
        check(lib.cnerf_view_colors_resolve(_p(state), _p(seen), M, _p(fallback), self._fill, _p(out), ptr(self.counts), stream()),
              "view_colors_resolve")
        return out

    def __call__(self, x, d):
        x, n = self._points(x, -d, "ViewColors")
        state, seen = self.accumulate(x, n)
        fb = None
        if self.fallback is not None:
            fb = self.fallback(x, d)
            if not torch.is_tensor(fb) or fb.dim() != 2 or fb.shape[0] != x.shape[0] or fb.shape[1] < 3 or not fb.is_floating_point():
                raise ValueError(f"ViewColors: fallback must return a floating tensor [N, >= 3] for N = {x.shape[0]} points, got "
                                 f"{tuple(fb.shape) if torch.is_tensor(fb) else type(fb).__name__}")
            fb = fb.detach()[:, :3].float().to(self.device).contiguous()
        return self.resolve(state, seen, fb)


def bvh_workspace_bytes(V, F):
    return _bytes("mesh_bvh", int(V), int(F))


_BVH_FLAGS = ((1, "a face index lies outside [0, V)"), (2, "a face has a non-finite coordinate"), (4, "a face needs more than 256^2 samples"))


class MeshBVH:
    """A triangle mesh indexed for closest-point queries (build_bvh): the workspace of cnerf_mesh_bvh_* (self-contained: it holds the
    triangles), V and F of the mesh it was built from, n_faces = the faces in the tree, and which faces were left out: bad_index (some
    index outside [0, V)), non_finite (some coordinate not finite).  moments / moments_nbytes: the buffer of cnerf_mesh_winding_build,
    None until winding_number, contains or signed_distance first asks for it."""

    def __init__(self, ws, nbytes, V, F, n_faces, flags):
        self.ws, self.nbytes, self.V, self.F, self.n_faces = ws, nbytes, V, F, n_faces
        self.moments, self.moments_nbytes = None, 0
        self.bad_index, self.non_finite = bool(flags & 1), bool(flags & 2)


def build_bvh(verts, faces):
    """Index a triangle mesh for closest_point() on the device (csrc/mesh_bvh.hip; the rules are in include/customnerf_hip.h,
    cnerf_mesh_bvh_*): the faces ordered along a Morton curve by a device radix sort, a balanced tree of boxes over leaves of four
    triangles.  CUDA tensors verts [V, 3], faces [F, 3] (int); any triangle mesh.  A face with an index outside [0, V) or a non-finite
    coordinate is left out and reported on the returned MeshBVH, not raised."""
    v, f, _ = _mesh_args(verts, faces, None, "build_bvh")
    V, F = v.shape[0], f.shape[0]
    ws, nbytes = _workspace(v.device, "mesh_bvh", V, F)
    counts = torch.empty(2, dtype=torch.int32, device=v.device)
    check(lib.cnerf_mesh_bvh_build(_p(v), V, _p(f), F, ptr(ws), nbytes, ptr(counts), stream()), "mesh_bvh_build")
    n, flags = _read(counts, "build_bvh", ())                                   # the one host read
    return MeshBVH(ws, nbytes, V, F, n, flags)


def closest_point(bvh, points, want_point=False, want_bary=False, want_stats=False):
    """The closest point of the mesh of `bvh` (build_bvh) to each of points [Q, 3] (CUDA float tensor), on the device.
    -> dict: dist2 [Q] float32 (squared distance), face [Q] int32 (the smallest face index at that distance; -1 with dist2 = +inf for a
    non-finite point or a mesh without valid faces), and on request point [Q, 3] (the closest point), bary [Q, 3] (its barycentrics in the
    face) and stats = (node boxes tested, triangles tested) summed over the call.  The result is the brute-force minimum over the faces
    under the float32 rule of include/customnerf_hip.h, bit for bit: the tree only prunes."""
    if not isinstance(bvh, MeshBVH):
        raise ValueError("closest_point: bvh must come from build_bvh")
    require_cuda(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"closest_point: points must be [Q, 3], got {tuple(points.shape)}")
    x = points.detach().contiguous().float()
    Q, dev = x.shape[0], x.device
    if Q >= 2 ** 31:
        raise ValueError(f"closest_point: at most 2^31 - 1 points per call, got {Q}")
    out = {'dist2': torch.empty(Q, dtype=torch.float32, device=dev), 'face': torch.empty(Q, dtype=torch.int32, device=dev)}
    if want_point:
        out['point'] = torch.empty(Q, 3, dtype=torch.float32, device=dev)
    if want_bary:
        out['bary'] = torch.empty(Q, 3, dtype=torch.float32, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev) if want_stats else None
    check(lib.cnerf_mesh_bvh_closest(ptr(bvh.ws), bvh.nbytes, bvh.V, bvh.F, _p(x), Q, _p(out['dist2']), _p(out['face']), _p(out.get('point')),
                                     _p(out.get('bary')), _p(stats), stream()), "mesh_bvh_closest")
    if want_stats:
        out['stats'] = tuple(int(s) for s in stats.cpu())
    return out


def _ray_args(bvh, origins, dirs, t_min, t_max, cull, what):
    """validated arguments of the ray queries -> (o, d, Q, t_min, t_max as floats, their [Q] tensors or None, the cull code)"""
    if not isinstance(bvh, MeshBVH):
        raise ValueError(f"{what}: bvh must come from build_bvh")
    if cull not in _CULL:
        raise ValueError(f"{what}: cull must be 'none', 'back' or 'front', got {cull!r}")
    for name, t in (("origins", origins), ("dirs", dirs)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: {name} must be a tensor on the GPU")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{what}: {name} must be [Q, 3], got {tuple(t.shape)}")
    if origins.shape[0] != dirs.shape[0]:
        raise ValueError(f"{what}: origins and dirs must have one row per ray, got {origins.shape[0]} and {dirs.shape[0]}")
    o, d = origins.detach().contiguous().float(), dirs.detach().contiguous().float()
    Q = o.shape[0]
    if Q >= 2 ** 31:
        raise ValueError(f"{what}: at most 2^31 - 1 rays per call, got {Q}")
    lim, per = [], []
    for name, t in (("t_min", t_min), ("t_max", t_max)):
        if torch.is_tensor(t):
            if not t.is_cuda or tuple(t.shape) != (Q,):
                raise ValueError(f"{what}: {name} must be a number or a [Q] tensor on the GPU, got {tuple(t.shape)} on {t.device}")
            lim.append(0.0)
            per.append(t.detach().contiguous().float())
        else:
            lim.append(float(t))
            per.append(None)
    return o, d, Q, lim[0], lim[1], per[0], per[1], _CULL[cull]


def ray_cast(bvh, origins, dirs, t_min=0.0, t_max=math.inf, cull='none', want_bary=False, want_stats=False):
    """The first face of the mesh of `bvh` (build_bvh) that each ray origins[q] + t dirs[q] meets with t_min <= t <= t_max, on the device
    (csrc/mesh_bvh.hip, k_bvh_raycast).  origins, dirs [Q, 3] CUDA float tensors; dirs are not normalised and t is in units of |dirs[q]|;
    t_min / t_max are numbers or [Q] CUDA tensors; cull 'none', 'back' or 'front' as in rasterize (faces wound outwards are front-facing
    from outside).  -> dict: t [Q] float32 (+inf: a miss), face [Q] int32 (the smallest face index at that t; -1: a miss), and on request
    bary [Q, 3] (the hit's barycentrics in the face; 0 for a miss) and stats = (node boxes tested, triangles tested) summed over the call.
    The ray/triangle test is the watertight one of Woop, Benthin and Wald (the rule is in include/customnerf_hip.h, cnerf_mesh_bvh_raycast):
    a ray through a shared edge or vertex hits one of the faces around it.  The result is the brute-force answer under that float32 rule,
    bit for bit: the tree only prunes.  A ray with a non-finite origin, a zero or non-finite direction or t_min > t_max misses.  Rays next
    to each other in the batch should be next to each other in space: they walk the tree together.  Bad arguments raise ValueError."""
    o, d, Q, t0, t1, p0, p1, c = _ray_args(bvh, origins, dirs, t_min, t_max, cull, "ray_cast")
    dev = o.device
    out = {'t': torch.empty(Q, dtype=torch.float32, device=dev), 'face': torch.empty(Q, dtype=torch.int32, device=dev)}
    if want_bary:
        out['bary'] = torch.empty(Q, 3, dtype=torch.float32, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev) if want_stats else None
    check(lib.cnerf_mesh_bvh_raycast(ptr(bvh.ws), bvh.nbytes, bvh.V, bvh.F, _p(o), _p(d), Q, t0, t1, _p(p0), _p(p1), c, _p(out['t']),
                                     _p(out['face']), _p(out.get('bary')), _p(stats), stream()), "mesh_bvh_raycast")
    if want_stats:
        out['stats'] = tuple(int(s) for s in stats.cpu())
    return out


def occluded(bvh, origins, dirs, t_min=0.0, t_max=math.inf, cull='none'):
    """Whether some face of the mesh of `bvh` stops each ray within [t_min, t_max]: ray_cast(...)['face'] >= 0 without the search for the
    first hit (csrc/mesh_bvh.hip, k_bvh_occluded, which leaves the tree at the first face it accepts).  Arguments as ray_cast.
    -> [Q] bool on the device."""
    o, d, Q, t0, t1, p0, p1, c = _ray_args(bvh, origins, dirs, t_min, t_max, cull, "occluded")
    occ = torch.empty(Q, dtype=torch.uint8, device=o.device)
    check(lib.cnerf_mesh_bvh_occluded(ptr(bvh.ws), bvh.nbytes, bvh.V, bvh.F, _p(o), _p(d), Q, t0, t1, _p(p0), _p(p1), c, _p(occ), None,
                                      stream()), "mesh_bvh_occluded")
    return occ != 0


def winding_workspace_bytes(V, F):
    return _bytes("mesh_winding", int(V), int(F))


def _moments(bvh):
    """the per-node moments of `bvh` that the winding walk reads (cnerf_mesh_winding_build), made on first use and kept on the MeshBVH"""
    if bvh.moments is None:
        mom, nbytes = _workspace(bvh.ws.device, "mesh_winding", bvh.V, bvh.F)
        check(lib.cnerf_mesh_winding_build(ptr(bvh.ws), bvh.nbytes, bvh.V, bvh.F, ptr(mom), nbytes, stream()), "mesh_winding_build")
        bvh.moments, bvh.moments_nbytes = mom, nbytes
    return bvh.moments, bvh.moments_nbytes


def _winding_args(bvh, points, beta, what):
    if not isinstance(bvh, MeshBVH):
        raise ValueError(f"{what}: bvh must come from build_bvh")
    beta = float(beta)
    if not beta >= 1.0:
        raise ValueError(f"{what}: beta must be >= 1 (math.inf: the exact sum), got {beta}")
    require_cuda(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points must be [Q, 3], got {tuple(points.shape)}")
    x = points.detach().contiguous().float()
    if x.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: at most 2^31 - 1 points per call, got {x.shape[0]}")
    return x, x.shape[0], beta


def winding_number(bvh, points, beta=2.0, want_stats=False):
    """The generalized winding number of the mesh of `bvh` (build_bvh) about each of points [Q, 3] (CUDA float tensor), on the device
    (csrc/mesh_bvh.hip, k_bvh_winding; the rule is in include/customnerf_hip.h, cnerf_mesh_winding_query) -> [Q] float32: 1 inside a
    closed mesh wound outwards, 0 outside, 2 where two such meshes overlap, -1 inside one wound inwards, and a smooth blend of these
    across a hole or next to a non-manifold edge, which is what makes it a usable inside test for meshes that are not watertight.
    A part of the mesh further from the point than `beta` times its radius is taken whole as one dipole (Barill et al. 2018) from
    moments kept per tree node; they are built on first use and cached on `bvh` as .moments.  beta=2.0 is the paper's choice, not an
    optimum measured here; beta=math.inf evaluates every face: the exact sum, in float32.  0 for a non-finite point or a mesh without
    valid faces.  want_stats: -> (w, (nodes accepted whole, triangles evaluated)) summed over the call."""
    x, Q, beta = _winding_args(bvh, points, beta, "winding_number")
    mom, mom_bytes = _moments(bvh)
    w = torch.empty(Q, dtype=torch.float32, device=x.device)
    stats = torch.zeros(2, dtype=torch.int64, device=x.device) if want_stats else None
    check(lib.cnerf_mesh_winding_query(ptr(bvh.ws), bvh.nbytes, bvh.V, bvh.F, ptr(mom), mom_bytes, _p(x), Q, beta, _p(w), _p(stats), stream()),
          "mesh_winding_query")
    return (w, tuple(int(s) for s in stats.cpu())) if want_stats else w


def contains(bvh, points, beta=2.0):
    """Whether each of points [Q, 3] lies inside the mesh of `bvh`: winding_number(bvh, points, beta) >= 0.5 -> [Q] bool on the device."""
    return winding_number(bvh, points, beta) >= 0.5


def signed_distance(bvh, points, beta=2.0, want_winding=False, want_stats=False):
    """The signed distance from each of points [Q, 3] (CUDA float tensor) to the mesh of `bvh` (build_bvh), negative inside, in one
    kernel (csrc/mesh_bvh.hip, k_bvh_signed): the closest-point walk of closest_point, unchanged, gives the magnitude and the face, the
    walk of winding_number the sign.  -> dict: signed [Q] float32 = -sqrt(dist2) where the winding number is >= 0.5, else sqrt(dist2);
    face [Q] int32 as closest_point returns it; on request winding [Q] float32 and stats = (nodes accepted whole, triangles evaluated)
    of the winding walk.  A non-finite point or a mesh without valid faces: signed = +inf, face = -1.  beta as in winding_number (2.0 is
    the paper's choice, not measured here)."""
    x, Q, beta = _winding_args(bvh, points, beta, "signed_distance")
    mom, mom_bytes = _moments(bvh)
    dev = x.device
    out = {'signed': torch.empty(Q, dtype=torch.float32, device=dev), 'face': torch.empty(Q, dtype=torch.int32, device=dev)}
    if want_winding:
        out['winding'] = torch.empty(Q, dtype=torch.float32, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev) if want_stats else None
    check(lib.cnerf_mesh_bvh_signed_distance(ptr(bvh.ws), bvh.nbytes, bvh.V, bvh.F, ptr(mom), mom_bytes, _p(x), Q, beta, _p(out['signed']),
                                             _p(out['face']), _p(out.get('winding')), _p(stats), stream()), "mesh_bvh_signed_distance")
    if want_stats:
        out['stats'] = tuple(int(s) for s in stats.cpu())
    return out


def voxel_remesh(verts, faces, resolution=None, voxel=None, offset=0.0, beta=2.0, probe=2, pad=2, chunk=2 ** 21):
    """A new mesh of the surface {signed_distance == offset} of the mesh (verts [V, 3], faces [F, 3], CUDA tensors), extracted by
    marching cubes over a cubic lattice: sparse_volume over the field -signed_distance, then marching_cubes_sparse at the level -offset
    (inside is value >= level, the rule of marching_cubes).  Exactly one of `resolution` (the number of lattice points along the longest
    side of the box) and `voxel` (the step) is given; the lattice covers the box of the faces that take part (finite coordinates, valid
    indices), grown by ceil(|offset| / step) + pad steps on every side.  offset > 0 thickens the surface, offset < 0 shrinks it, in the
    units of verts.  beta as in winding_number; probe and chunk as in sparse_volume, which documents what probe > 1 can miss (probe=1
    misses nothing).
    -> (verts, faces, normals, info): info holds shape, origin, spacing, bricks, evaluations, rounds, offset and beta.
    What this is: the output is closed and manifold wherever the level set is regular, whatever the input — holes are capped along the
    surface where the winding number is 0.5, faces inside the union of overlapping closed parts vanish, non-manifold edges go.  What it is
    not: detail below a voxel is lost and every vertex moves (by less than a step); sharp edges are rounded; a closed mesh wound inwards
    has winding number -1 inside, counts as outside everywhere and comes out empty."""
    what = "voxel_remesh"
    if (resolution is None) == (voxel is None):
        raise ValueError(f"{what}: give exactly one of resolution and voxel")
    offset, pad = float(offset), int(pad)
    if not math.isfinite(offset) or pad < 1:
        raise ValueError(f"{what}: offset must be finite and pad >= 1, got {offset} and {pad}")
    if not float(beta) >= 1.0:
        raise ValueError(f"{what}: beta must be >= 1 (math.inf: the exact sum), got {beta}")
    if resolution is not None and int(resolution) < 2:
        raise ValueError(f"{what}: resolution must be >= 2, got {resolution}")
    if voxel is not None and not (float(voxel) > 0.0 and math.isfinite(float(voxel))):
        raise ValueError(f"{what}: voxel must be positive and finite, got {voxel}")
    v, f, _ = _mesh_args(verts, faces, None, what)
    bvh = build_bvh(v, f)
    empty = (torch.empty(0, 3, dtype=torch.float32, device=v.device), torch.empty(0, 3, dtype=torch.int32, device=v.device),
             torch.empty(0, 3, dtype=torch.float32, device=v.device))
    info = {'shape': (0, 0, 0), 'origin': (0.0, 0.0, 0.0), 'spacing': (0.0, 0.0, 0.0), 'bricks': 0, 'evaluations': 0, 'rounds': 0,
            'offset': offset, 'beta': float(beta)}
    if not bvh.n_faces:
        return empty + (info,)
    fi = f.long()
    tri = v[fi[((fi >= 0) & (fi < v.shape[0])).all(1)]]                        # [n, 3, 3]
    p = tri[torch.isfinite(tri).all(2).all(1)].reshape(-1, 3)
    lo, hi = (t.double().cpu() for t in (p.min(0).values, p.max(0).values))     # a host read: the lattice's shape depends on it
    side = float((hi - lo).max())
    h = side / (int(resolution) - 1) if resolution is not None else float(voxel)
    if not (h > 0.0 and math.isfinite(h)):
        raise ValueError(f"{what}: the step must be positive and finite, got {h} (a mesh of one point needs voxel=)")
    grow = math.ceil(abs(offset) / h - 1e-9) + pad
    shape = tuple(int(math.ceil(float(hi[a] - lo[a]) / h - 1e-9)) + 1 + 2 * grow for a in range(3))
    origin = tuple(float(lo[a]) - grow * h for a in range(3))
    _shape3(shape, what)
    sv = sparse_volume(lambda x: -signed_distance(bvh, x, beta)['signed'], shape, origin, (h, h, h), -offset, probe=probe, chunk=chunk,
                       device=v.device)
    info.update(shape=shape, origin=sv.origin, spacing=sv.spacing, bricks=sv.n_bricks, evaluations=sv.evaluations, rounds=sv.rounds)
    return marching_cubes_sparse(sv, -offset) + (info,)


class BakeSource:
    """A mesh to bake from (bake_source): bvh, the MeshBVH of its faces; faces [F, 3] int32 and normals [V, 3] float32 or None, contiguous,
    on the device — what project_to_surface reads beyond the tree; diagonal, the diagonal of the box of the faces that take part (0.0
    without any)."""

    def __init__(self, bvh, faces, normals, diagonal):
        self.bvh, self.faces, self.normals, self.diagonal = bvh, faces, normals, diagonal


def bake_source(verts, faces, normals=None):
    """Index a (full-resolution) mesh as the surface that project_to_surface and bake_texture(source=) project onto: build_bvh plus the
    faces and the vertex normals, from which the projected points' normals are interpolated (without normals they are the faces' own).
    CUDA tensors verts [V, 3], faces [F, 3] (int), normals [V, 3] or None -> BakeSource.  Faces left out of the tree (build_bvh) are
    never projected onto."""
    v, f, n = _mesh_args(verts, faces, normals, "bake_source")
    bvh = build_bvh(v, f)
    diag = 0.0
    if bvh.n_faces:
        lo, hi = torch.aminmax(v[_used_mask(v, f)], dim=0)
        diag = float((hi - lo).double().norm())
    return BakeSource(bvh, f, n, diag)


def project_to_surface(source, points, normals, reach, want_stats=False):
    """Project points [Q, 3] onto the surface of `source` (bake_source) along their normals [Q, 3] (the outward normals of the mesh the
    points lie on; not normalised), at most `reach` away (a number > 0, or a [Q] CUDA tensor), on the device (csrc/mesh_bvh.hip,
    k_bvh_project; the rule is in include/customnerf_hip.h, cnerf_mesh_bvh_project).  Two rays leave each point: along the normal, accepting
    only source faces that look the way the normal does (met from behind), and against it, accepting only faces that look back at it; the
    nearer hit wins, so a point of a thin part never lands on the opposite wall.  Where both miss (past a rim), the closest point of the
    source is taken when it lies within reach.  -> dict: point [Q, 3] (the projected point; the input point where nothing was found),
    normal [Q, 3] (unit: the source's normal there, interpolated from its vertex normals, else its face's; the input normal normalised
    where nothing was found), offset [Q] (the signed distance moved along the normal, in units of its length), face [Q] int32 (the source
    face, -1: none), kind [Q] uint8 (0 nothing found, 1 along the normal, 2 against it, 3 closest point) and on request stats = (node
    boxes tested, triangles tested) summed over the call.  The result is the brute-force answer under the float32 rule, bit for bit.
    Points next to each other in the batch should be next to each other in space.  Bad arguments raise ValueError."""
    what = "project_to_surface"
    if not isinstance(source, BakeSource):
        raise ValueError(f"{what}: source must come from bake_source")
    for name, t in (("points", points), ("normals", normals)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: {name} must be a tensor on the GPU")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{what}: {name} must be [Q, 3], got {tuple(t.shape)}")
    if points.shape[0] != normals.shape[0]:
        raise ValueError(f"{what}: points and normals must have one row per query, got {points.shape[0]} and {normals.shape[0]}")
    x, n = points.detach().contiguous().float(), normals.detach().contiguous().float()
    Q, dev = x.shape[0], x.device
    if Q >= 2 ** 31:
        raise ValueError(f"{what}: at most 2^31 - 1 queries per call, got {Q}")
    if torch.is_tensor(reach):
        if not reach.is_cuda or tuple(reach.shape) != (Q,):
            raise ValueError(f"{what}: reach must be a number or a [Q] tensor on the GPU, got {tuple(reach.shape)} on {reach.device}")
        r0, per = 0.0, reach.detach().contiguous().float()
    else:
        r0, per = float(reach), None
        if not r0 > 0.0:
            raise ValueError(f"{what}: reach must be > 0, got {reach}")
    out = {'point': torch.empty(Q, 3, dtype=torch.float32, device=dev), 'normal': torch.empty(Q, 3, dtype=torch.float32, device=dev),
           'offset': torch.empty(Q, dtype=torch.float32, device=dev), 'face': torch.empty(Q, dtype=torch.int32, device=dev),
           'kind': torch.empty(Q, dtype=torch.uint8, device=dev)}
    stats = torch.zeros(2, dtype=torch.int64, device=dev) if want_stats else None
    bvh = source.bvh
    check(lib.cnerf_mesh_bvh_project(ptr(bvh.ws), bvh.nbytes, bvh.V, bvh.F, _p(source.faces), _p(source.normals), _p(x), _p(n), Q, r0, _p(per),
                                     _p(out['point']), _p(out['normal']), _p(out['offset']), _p(out['face']), _p(out['kind']), _p(stats),
                                     stream()), "mesh_bvh_project")
    if want_stats:
        out['stats'] = tuple(int(s) for s in stats.cpu())
    return out


def ao_directions(K):
    """K fixed directions on the hemisphere about +z, cosine-weighted (their density is proportional to z), as [K, 3] float32 on the host:
    spherical-Fibonacci points, for i = 0 .. K - 1: u = (i + 0.5) / K, z = sqrt(1 - u), r = sqrt(u), phi = 2 pi frac(i (sqrt(5) - 1) / 2),
    direction (r cos phi, r sin phi, z), computed in float64 and rounded once."""
    K = int(K)
    if K < 1:
        raise ValueError(f"ao_directions: need K >= 1, got {K}")
    i = np.arange(K, dtype=np.float64)
    u = (i + 0.5) / float(K)
    phi = 2.0 * math.pi * np.mod(i * ((math.sqrt(5.0) - 1.0) / 2.0), 1.0)
    r = np.sqrt(u)
    return torch.from_numpy(np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u)], 1).astype(np.float32))


def ao_rays(verts, normals, dirs, bias):
    """The ambient-occlusion rays of vertices verts [N, 3] with normals [N, 3] for hemisphere directions dirs [K, 3] (ao_directions), in
    torch float32 on the device -> (origins [N, K, 3], directions [N, K, 3]).  n = normals / sqrt((nx nx + ny ny) + nz nz); the frame is
    the branch-free orthonormal basis of Duff et al. (JCGT 6(1), 2017): s = copysign(1, nz), a = -1 / (s + nz), b = (nx ny) a,
    b1 = (1 + (s (nx nx)) a, s b, -s nx), b2 = (b, s + (ny ny) a, -ny); direction = (dx b1 + dy b2) + dz n, origin = x + bias n."""
    n = normals / ((normals[:, 0:1] * normals[:, 0:1] + normals[:, 1:2] * normals[:, 1:2]) + normals[:, 2:3] * normals[:, 2:3]).sqrt()
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    s = torch.copysign(torch.ones_like(nz), nz)
    a = -1.0 / (s + nz)
    b = (nx * ny) * a
    b1 = torch.stack([1.0 + (s * (nx * nx)) * a, s * b, (-s) * nx], 1)
    b2 = torch.stack([b, s + (ny * ny) * a, -ny], 1)
    d = dirs.to(n.device)
    out = (d[None, :, 0:1] * b1[:, None] + d[None, :, 1:2] * b2[:, None]) + d[None, :, 2:3] * n[:, None]
    org = verts + bias * n
    return org[:, None].expand_as(out), out


def ambient_occlusion(verts, faces, normals=None, samples=64, radius=None, bias=None, chunk=2 ** 22):
    """Per-vertex ambient occlusion of a triangle mesh, as mesh viewers compute it, on the device: the share of `samples` rays from each
    vertex that no face of the mesh stops.  The rays start at x + bias n (bias: by default 1e-4 of the diagonal of the mesh's box) and
    follow ao_directions(samples) turned into the vertex's frame (ao_rays); a face stops a ray when it is hit at 0 <= t <= radius (by
    default: anywhere).  Without `normals`, vertex_normals(verts, faces).  -> [V] float32 in [0, 1]; 1 for a vertex no valid face uses.
    A composition over occluded() on build_bvh(verts, faces), at most `chunk` rays at a time.  CUDA tensors verts [V, 3], faces [F, 3]
    (int), normals [V, 3] or None.  samples < 1, a non-finite bias, a radius that is not > 0 or chunk < 1 raise ValueError."""
    for name, t in (("verts", verts), ("faces", faces), ("normals", normals)):
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise ValueError(f"ambient_occlusion: {name} must be a tensor on the GPU")
    v, f, n = _mesh_args(verts, faces, normals, "ambient_occlusion")
    K, chunk = int(samples), int(chunk)
    if K < 1:
        raise ValueError(f"ambient_occlusion: samples must be >= 1, got {samples}")
    if chunk < 1:
        raise ValueError(f"ambient_occlusion: chunk must be >= 1, got {chunk}")
    radius = math.inf if radius is None else float(radius)
    if not radius > 0.0:
        raise ValueError(f"ambient_occlusion: radius must be > 0, got {radius}")
    if bias is not None and not math.isfinite(float(bias)):
        raise ValueError(f"ambient_occlusion: bias must be finite, got {bias}")
    V, dev = v.shape[0], v.device
    ao = torch.ones(V, dtype=torch.float32, device=dev)
    bvh = build_bvh(v, f)
    if V == 0 or bvh.n_faces == 0:
        return ao
    mask = _used_mask(v, f)
    if bias is None:
        lo, hi = torch.aminmax(v[mask], dim=0)
        bias = 1e-4 * float((hi - lo).double().norm())
    bias = float(bias)
    if n is None:
        n = vertex_normals(v, f)
    dirs = ao_directions(K).to(dev)
    kb = min(K, chunk)
    vb = max(1, chunk // kb)
    free = torch.zeros(V, dtype=torch.int64, device=dev)
    for v0 in range(0, V, vb):
        for k0 in range(0, K, kb):
            org, d = ao_rays(v[v0:v0 + vb], n[v0:v0 + vb], dirs[k0:k0 + kb], bias)
            occ = occluded(bvh, org.reshape(-1, 3), d.reshape(-1, 3), 0.0, radius)
            free[v0:v0 + vb] += (~occ).reshape(org.shape[0], -1).sum(1)
    ao[mask] = free[mask].float() / float(K)
    return ao


def _sample(verts, faces, spacing, max_samples, what):
    """the sampler behind sample_surface and distance -> ((points, face, bary, weight), flags); a face that needs k > 256 is sampled at
    k = 256 and sets flags bit 2: the caller decides"""
    v, f, _ = _mesh_args(verts, faces, None, what)
    sp = float(np.float32(spacing))
    if not (math.isfinite(sp) and sp > 0.0):
        raise ValueError(f"{what}: spacing must be finite and > 0, got {spacing}")
    V, F, dev = v.shape[0], f.shape[0], v.device
    ws, nbytes = _workspace(dev, "mesh_sample", F)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    check(lib.cnerf_mesh_sample_count(_p(v), V, _p(f), F, sp, ptr(ws), nbytes, ptr(counts), stream()), "mesh_sample_count")
    n, flags = (int(c) for c in counts.cpu())                                   # the one host read
    if n > int(max_samples):
        raise ValueError(f"{what}: {n} samples at spacing {sp} exceed max_samples = {max_samples}")
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    bary = torch.empty(n, 3, dtype=torch.float32, device=dev)
    weight = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib.cnerf_mesh_sample_emit(_p(v), V, _p(f), F, sp, ptr(ws), nbytes, _p(pts), _p(face), _p(bary), _p(weight), n, stream()),
          "mesh_sample_emit")
    return (pts, face, bary, weight), flags


def sample_surface(verts, faces, spacing, max_samples=1 << 26):
    """Deterministic samples of a mesh's surface about `spacing` apart, on the device (csrc/mesh_bvh.hip, cnerf_mesh_sample_*): a face of
    area A is cut into k^2 congruent triangles, k = ceil(sqrt(2 A) / spacing) in [1, 256], with one sample at the centroid of each,
    weighted A / k^2; faces with a bad index or a non-finite coordinate give none.  -> (points [n, 3] float32, face [n] int32,
    bary [n, 3] float32, weight [n] float32) in face order.  More than max_samples samples, or a face that needs k > 256, raises ValueError."""
    out, flags = _sample(verts, faces, spacing, max_samples, "sample_surface")
    if flags & 4:
        raise ValueError(f"sample_surface: {_BVH_FLAGS[2][1]} at spacing {spacing} (a larger spacing)")
    return out


def _used_mask(v, f):
    """[V] bool: the vertices of the faces that take part (valid indices, finite coordinates)"""
    V = v.shape[0]
    fl = f.long()
    ok = ((fl >= 0) & (fl < V)).all(1)
    fl = fl[ok]
    fl = fl[torch.isfinite(v[fl.reshape(-1)]).reshape(-1, 9).all(1)]
    used = torch.zeros(V, dtype=torch.bool, device=v.device)
    used[fl.reshape(-1)] = True
    return used


def _used_vertices(v, f):
    """the vertices of the faces that take part, in index order"""
    return v[_used_mask(v, f)]


def _one_way(v, f, bvh, spacing, include_vertices, max_samples):
    (pts, _, _, w), _ = _sample(v, f, spacing, max_samples, "distance")          # a face that needs k > 256 gets k = 256: its weights still sum to its area
    n = pts.shape[0]
    if include_vertices:
        extra = _used_vertices(v, f)
        pts = torch.cat([pts, extra])
        w = torch.cat([w, torch.zeros(extra.shape[0], dtype=torch.float32, device=v.device)])
    if pts.shape[0] == 0:
        raise ValueError("distance: a mesh has no face to sample")
    r = closest_point(bvh, pts)
    d2, w = r['dist2'].double(), w.double()
    i = int(torch.nonzero(r['dist2'] == r['dist2'].max())[0])                    # the first sample at the maximum
    area = float(w.sum())
    mean = float((w * d2.sqrt()).sum()) / area if area > 0.0 else 0.0
    rms = math.sqrt(float((w * d2).sum()) / area) if area > 0.0 else 0.0
    return {'max': math.sqrt(float(d2[i])), 'mean': mean, 'rms': rms, 'n_samples': n, 'max_point': tuple(float(c) for c in pts[i]),
            'max_face': int(r['face'][i])}


def distance(verts_a, faces_a, verts_b, faces_b, spacing=None, symmetric=True, include_vertices=True, max_samples=1 << 26):
    """Geometric deviation between two triangle meshes, as Metro and MeshLab report it, on the device: A's surface is sampled about
    `spacing` apart (sample_surface; default 0.002 x the diagonal of the box around both meshes) and each sample's distance to B comes
    from closest_point on B's tree; with symmetric=True also B to A.  A face so large that it would need more than 256^2 samples gets
    256^2.  include_vertices adds the sampled mesh's vertices with weight 0: they count for the maximum only (extremes sit at vertices).
    CUDA tensors verts [V, 3], faces [F, 3] (int) per mesh; at most max_samples samples per direction (ValueError beyond).
    -> dict: 'a_to_b' (and 'b_to_a'): max, mean and rms (area-weighted, summed in float64) in the meshes' units, n_samples, max_point (the
    sample where the maximum is attained) and max_face (the face of the other mesh closest to it); 'hausdorff' = the largest max;
    'spacing'.  A mesh without a valid face raises ValueError."""
    va, fa, _ = _mesh_args(verts_a, faces_a, None, "distance")
    vb, fb, _ = _mesh_args(verts_b, faces_b, None, "distance")
    if spacing is None:
        both = torch.cat([va, vb])
        both = both[torch.isfinite(both).all(1)]
        if both.shape[0] == 0:
            raise ValueError("distance: no finite vertex")
        lo, hi = torch.aminmax(both, dim=0)
        spacing = 0.002 * float((hi - lo).double().norm())
    spacing = float(spacing)
    if not (math.isfinite(spacing) and spacing > 0.0):
        raise ValueError(f"distance: spacing must be finite and > 0, got {spacing}")
    out = {'spacing': spacing}
    for key, (v, f), (tv, tf) in (('a_to_b', (va, fa), (vb, fb)), ('b_to_a', (vb, fb), (va, fa)))[:2 if symmetric else 1]:
        bvh = build_bvh(tv, tf)
        if bvh.n_faces == 0:
            raise ValueError("distance: a mesh has no valid face to measure against")
        out[key] = _one_way(v, f, bvh, spacing, include_vertices, max_samples)
    out['hausdorff'] = max(out[k]['max'] for k in ('a_to_b', 'b_to_a') if k in out)
    return out


def png_bytes(image, what="png_bytes"):
    """The bytes of an 8-bit RGB PNG (no interlace, filter 0 on every row), standard library only.  image: [H, W, 3] uint8 tensor (any
    device) or array."""
    a = _host(image, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{what}: image must be [H, W, 3] uint8, got {a.shape}")
    H, W = a.shape[:2]
    raw = np.zeros((H, 1 + 3 * W), dtype=np.uint8)                              # a filter-type byte (0) in front of every row
    raw[:, 1:] = a.reshape(H, 3 * W)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    return b"".join((b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)),
                     chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)), chunk(b"IEND", b"")))


def write_png(path, image):
    """8-bit RGB PNG (png_bytes) written to `path`.  image: [H, W, 3] uint8 tensor (any device) or array."""
    data = png_bytes(image, "write_png")
    with open(path, "wb") as fh:
        fh.write(data)


def write_apng(path, frames, fps=30, loop=0):
    """Animated PNG (APNG 1.0) of 8-bit RGB frames written to `path`, standard library only: the one-file stand-in for a video that
    browsers and image viewers open (a viewer that does not know APNG shows frame 0).  frames: a sequence of [H, W, 3] uint8 tensors
    (any device) or arrays, or one [N, H, W, 3]; every frame is shown 1 / fps seconds; loop = 0 repeats for ever.  Layout: IHDR, acTL
    (frame count, loop count), then fcTL + IDAT for frame 0 and fcTL + fdAT for every later one — full frames, no blending, filter 0 on
    every row — with ONE running sequence number over the fcTL and fdAT chunks, then IEND.  A single frame is accepted.
    ValueError: no frame, a frame that is not [H, W, 3] uint8 (floating-point frames are not converted here), frames of different
    sizes, fps or loop out of range."""
    if torch.is_tensor(frames) or isinstance(frames, np.ndarray):
        frames = list(frames)
    arrs = []
    for i, f in enumerate(frames):
        if (f.dtype != torch.uint8) if torch.is_tensor(f) else (np.asarray(f).dtype != np.uint8):
            raise ValueError(f"write_apng: frame {i} must be uint8, got {f.dtype if hasattr(f, 'dtype') else type(f)}")
        a = _host(f, np.uint8)
        if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] == 0 or a.shape[1] == 0:
            raise ValueError(f"write_apng: frame {i} must be [H, W, 3] uint8, got {a.shape}")
        if arrs and a.shape != arrs[0].shape:
            raise ValueError(f"write_apng: frame {i} is {a.shape}, frame 0 is {arrs[0].shape}")
        arrs.append(a)
    if not arrs:
        raise ValueError("write_apng: no frames")
    fps, loop = int(fps), int(loop)
    if not (1 <= fps <= 65535) or loop < 0:
        raise ValueError(f"write_apng: fps must be in [1, 65535] and loop >= 0, got {fps}, {loop}")
    H, W = arrs[0].shape[:2]

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    out = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)), chunk(b"acTL", struct.pack(">II", len(arrs), loop))]
    seq = 0
    for i, a in enumerate(arrs):
        # fcTL: sequence, width, height, x and y offset, delay numerator / denominator (seconds), dispose_op 0 (none), blend_op 0 (source)
        out.append(chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, 1, fps, 0, 0)))
        seq += 1
        raw = np.zeros((H, 1 + 3 * W), dtype=np.uint8)                          # a filter-type byte (0) in front of every row
        raw[:, 1:] = a.reshape(H, 3 * W)
        data = zlib.compress(raw.tobytes(), 6)
        if i == 0:
            out.append(chunk(b"IDAT", data))
        else:
            out.append(chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(chunk(b"IEND", b""))
    with open(path, "wb") as fh:
        fh.write(b"".join(out))


def write_glb(path, positions, indices, normals=None, uvs=None, tangents=None, colors=None, texture=None, normal_map=None, unlit=None):
    """glTF 2.0 binary (.glb): one mesh with one indexed triangle primitive and one material, everything in one file; json, struct and
    zlib only.  positions [W, 3] float32, indices [F, 3] (any int type; written as UNSIGNED_INT), and per vertex, all optional: normals
    [W, 3], uvs [W, 2] (already (u, 1 - v), as gltf_vertices gives them), tangents [W, 4] (xyz and the sign), colors [W, 3] uint8
    (COLOR_0, normalised RGBA8 with alpha 255).  texture and normal_map [R, R, 3] uint8 are embedded as PNG images (png_bytes): the
    material's baseColorTexture (metallicFactor 0, roughnessFactor 1) and its normalTexture, a tangent-space map as
    bake_texture(normal_map='tangent') makes it.  unlit=None: KHR_materials_unlit when there is no normal map (a NeRF's radiance already
    holds the shading), lit with one; a bool decides.  The file is a 12-byte header, the JSON chunk padded with spaces and the BIN chunk
    padded with zeros; every bufferView starts on a multiple of 4.  Accepts tensors (any device) or arrays.  ValueError: a normal map
    without tangents and uvs, a texture without uvs, a per-vertex array whose first dimension is not W, an index outside [0, W)."""
    import json
    pos = _host(positions, np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"write_glb: positions must be [W, 3], got {pos.shape}")
    W = len(pos)
    idx = _host(indices.view(torch.int32) if torch.is_tensor(indices) and indices.dtype == getattr(torch, 'uint32', None) else indices,
                np.int64).reshape(-1, 3)
    if idx.size and (idx.min() < 0 or idx.max() >= W):
        raise ValueError(f"write_glb: an index lies outside [0, W) for W = {W}")
    per_vertex = {}
    for name, a, cols, dt in (("normals", normals, 3, np.float32), ("uvs", uvs, 2, np.float32), ("tangents", tangents, 4, np.float32),
                              ("colors", colors, 3, np.uint8)):
        if a is None:
            continue
        a = _host(a, dt)
        if a.ndim != 2 or a.shape != (W, cols):
            raise ValueError(f"write_glb: {name} must be [W, {cols}] for W = {W} vertices, got {a.shape}")
        per_vertex[name] = a
    if texture is not None and "uvs" not in per_vertex:
        raise ValueError("write_glb: a texture needs uvs")
    if normal_map is not None and not ("uvs" in per_vertex and "tangents" in per_vertex):
        raise ValueError("write_glb: a normal map needs tangents and uvs (glTF takes tangent-space maps only)")
    if unlit is None:
        unlit = normal_map is None
    views, accessors, blob = [], [], bytearray()

    def view(data, target=None):
        blob.extend(b"\0" * (-len(blob) % 4))
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(data)})
        if target is not None:
            views[-1]["target"] = target
        blob.extend(data)
        return len(views) - 1

    def accessor(a, ctype, kind, target, **extra):
        accessors.append(dict({"bufferView": view(a.tobytes(), target), "componentType": ctype, "count": len(a), "type": kind}, **extra))
        return len(accessors) - 1

    prim = {"mode": 4, "indices": accessor(idx.astype("<u4").reshape(-1), 5125, "SCALAR", 34963)}
    bounds = {"min": pos.min(0).astype(np.float64).tolist(), "max": pos.max(0).astype(np.float64).tolist()} if W else \
        {"min": [0.0, 0.0, 0.0], "max": [0.0, 0.0, 0.0]}
    attr = {"POSITION": accessor(pos.astype("<f4"), 5126, "VEC3", 34962, **bounds)}
    for name, key, kind in (("normals", "NORMAL", "VEC3"), ("uvs", "TEXCOORD_0", "VEC2"), ("tangents", "TANGENT", "VEC4")):
        if name in per_vertex:
            attr[key] = accessor(per_vertex[name].astype("<f4"), 5126, kind, 34962)
    if "colors" in per_vertex:
        rgba = np.full((W, 4), 255, np.uint8)
        rgba[:, :3] = per_vertex["colors"]
        attr["COLOR_0"] = accessor(rgba, 5121, "VEC4", 34962, normalized=True)
    prim["attributes"] = attr
    pbr = {"metallicFactor": 0.0, "roughnessFactor": 1.0}
    material = {"pbrMetallicRoughness": pbr}
    images = []
    for img, what in ((texture, "texture"), (normal_map, "normal_map")):
        if img is None:
            continue
        images.append({"bufferView": view(png_bytes(img, f"write_glb: {what}")), "mimeType": "image/png"})
        slot = {"index": len(images) - 1, "texCoord": 0}
        if what == "texture":
            pbr["baseColorTexture"] = slot
        else:
            material["normalTexture"] = slot
    doc = {"asset": {"version": "2.0", "generator": "customnerf_amd"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}],
           "meshes": [{"primitives": [prim]}], "materials": [material], "accessors": accessors, "bufferViews": views}
    prim["material"] = 0
    if unlit:
        material["extensions"] = {"KHR_materials_unlit": {}}
        doc["extensionsUsed"] = ["KHR_materials_unlit"]
    if images:
        doc["images"] = images
        doc["samplers"] = [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
        doc["textures"] = [{"sampler": 0, "source": i} for i in range(len(images))]
    blob.extend(b"\0" * (-len(blob) % 4))
    doc["buffers"] = [{"byteLength": len(blob)}]
    js = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    js += b" " * (-len(js) % 4)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + 8 + len(blob)))
        fh.write(struct.pack("<I4s", len(js), b"JSON") + js)
        fh.write(struct.pack("<I4s", len(blob), b"BIN\0") + bytes(blob))


def _lines(fmt, a):
    """fmt applied to every row of the 2-D array a, as one string (one formatting call, no Python loop per row)"""
    return (fmt * len(a)) % tuple(a.ravel().tolist()) if len(a) else ""


def write_obj(path, verts, faces, uvs=None, normals=None, texture=None, normal_map=None):
    """Wavefront OBJ: `v x y z`, `vt u v` (three per face, in face order, when uvs [F, 3, 2] are given), `vn` (one per vertex, when normals
    [V, 3] are given) and `f v/vt/vn` lines, 1-based.  Floats are written with 9 significant digits, so float32 values read back exactly.
    With `texture` ([R, R, 3] uint8, needs uvs) the material goes to <stem>.mtl (map_Kd) and the image to <stem>.png beside the OBJ.
    With `normal_map` ([R, R, 3] uint8, needs uvs; object space, as bake_texture(normal_map=True) makes it) the image goes to
    <stem>_normal.png and a `norm <stem>_normal.png` line into the material.  Accepts tensors (any device) or arrays."""
    v = _host(verts, np.float32).reshape(-1, 3)
    f = _host(faces, np.int64).reshape(-1, 3)
    uv = _host(uvs, np.float32)
    n = _host(normals, np.float32)
    F = len(f)
    if uv is not None:
        uv = uv.reshape(-1, 2)
        if len(uv) != 3 * F:
            raise ValueError(f"write_obj: uvs must be [F, 3, 2] for F = {F} faces, got {len(uv)} corners")
    if n is not None:
        n = n.reshape(-1, 3)
        if len(n) != len(v):
            raise ValueError(f"write_obj: normals must be [V, 3] like verts, got {len(n)} for V = {len(v)}")
    if texture is not None and uv is None:
        raise ValueError("write_obj: a texture needs uvs")
    if normal_map is not None and uv is None:
        raise ValueError("write_obj: a normal map needs uvs")
    material = texture is not None or normal_map is not None
    if F and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("write_obj: a face index lies outside [0, V)")
    root, _ = os.path.splitext(path)
    stem = os.path.basename(root)
    head = ["# customnerf_amd mesh export", f"# {len(v)} vertices, {F} faces"]
    if material:
        head += [f"mtllib {stem}.mtl"]
    out = ["\n".join(head) + "\n", _lines("v %.9g %.9g %.9g\n", v.astype(np.float64))]
    if uv is not None:
        out.append(_lines("vt %.9g %.9g\n", uv.astype(np.float64)))
    if n is not None:
        out.append(_lines("vn %.9g %.9g %.9g\n", n.astype(np.float64)))
    if material:
        out.append("usemtl material0\n")
    vi = f + 1
    if uv is not None:
        ti = np.arange(1, 3 * F + 1, dtype=np.int64).reshape(F, 3)
        idx = np.stack([vi, ti, vi], -1) if n is not None else np.stack([vi, ti], -1)
        fmt = "/".join(["%d"] * idx.shape[2])
    elif n is not None:
        idx = np.stack([vi, vi], -1)
        fmt = "%d//%d"
    else:
        idx = vi[..., None]
        fmt = "%d"
    out.append(_lines(f"f {fmt} {fmt} {fmt}\n", idx.reshape(F, 3 * idx.shape[2])))
    with open(path, "w") as fh:
        fh.write("".join(out))
    if material:
        with open(root + ".mtl", "w") as fh:
            fh.write("newmtl material0\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\n" + (f"map_Kd {stem}.png\n" if texture is not None else "") +
                     (f"norm {stem}_normal.png\n" if normal_map is not None else ""))
    if texture is not None:
        write_png(root + ".png", texture)
    if normal_map is not None:
        write_png(root + "_normal.png", normal_map)
