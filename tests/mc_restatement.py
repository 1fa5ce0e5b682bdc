"""NumPy restatement of csrc/mesh.hip (count -> scan -> emit), on the table gen_mc_tables.py generates.  Test infrastructure only.

Same conventions as the kernels: corner inside <=> v >= level (NaN outside); vertex per crossing edge, owned by the edge's lower point,
ordered by (linear point index, axis); triangles ordered by (linear cell index, table order); float32 arithmetic in the kernels' order.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "customnerf_amd", "csrc")
if CSRC not in sys.path:
    sys.path.insert(0, CSRC)
import gen_mc_tables  # noqa: E402

TRI, NTRI = gen_mc_tables.build()
EDGE_CORNER = np.array([a for a, _, _ in gen_mc_tables.EDGES])
EDGE_AXIS = np.array([ax for _, _, ax in gen_mc_tables.EDGES])


def _shift(a, axis, lo):
    """a[..] restricted to [lo, lo + n - 1) along `axis` (lo in {0, 1})"""
    sl = [slice(None)] * 3
    sl[axis] = slice(lo, a.shape[axis] - 1 + lo)
    return a[tuple(sl)]


def _grad(vol, sp):
    """[3, nx, ny, nz]: central differences / spacing, one-sided on the faces (mesh.hip mc_grad)"""
    out = np.empty((3,) + vol.shape, dtype=np.float32)
    for b in range(3):
        v = np.moveaxis(vol, b, 0)
        g = np.empty_like(v)
        g[1:-1] = (v[2:] - v[:-2]) / (np.float32(2) * sp[b])
        g[0] = (v[1] - v[0]) / (np.float32(1) * sp[b])
        g[-1] = (v[-1] - v[-2]) / (np.float32(1) * sp[b])
        out[b] = np.moveaxis(g, 0, b)
    return out


def counts(vol, level):
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    inside = vol >= np.float32(level)
    nv = sum(int((_shift(inside, a, 0) != _shift(inside, a, 1)).sum()) for a in range(3))
    case = np.zeros(tuple(n - 1 for n in vol.shape), dtype=np.int64)
    for c in range(8):
        sl = tuple(slice((c >> a) & 1, vol.shape[a] - 1 + ((c >> a) & 1)) for a in range(3))
        case |= inside[sl].astype(np.int64) << c
    return nv, int(NTRI[case].sum())


def marching_cubes(vol, level, spacing=(1, 1, 1), origin=(0, 0, 0), normals=True):
    """-> verts [V,3] f32, faces [F,3] int32, normals [V,3] f32 | None"""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    n = vol.size
    level = np.float32(level)
    sp = np.asarray(spacing, dtype=np.float32)
    org = np.asarray(origin, dtype=np.float32)
    inside = vol >= level
    flat = vol.reshape(-1)
    strides = (ny * nz, nz, 1)
    # count: crossing mask of the owned edges, case of the cell at each point
    mask = np.zeros(vol.shape, dtype=np.int64)
    for a in range(3):
        cross = _shift(inside, a, 0) != _shift(inside, a, 1)
        sl = [slice(None)] * 3
        sl[a] = slice(0, vol.shape[a] - 1)
        mask[tuple(sl)] |= cross.astype(np.int64) << a
    case = np.zeros(vol.shape, dtype=np.int64)
    cell = (slice(0, nx - 1), slice(0, ny - 1), slice(0, nz - 1))
    for c in range(8):
        sl = tuple(slice((c >> a) & 1, vol.shape[a] - 1 + ((c >> a) & 1)) for a in range(3))
        case[cell] |= inside[sl].astype(np.int64) << c
    mask, case = mask.reshape(-1), case.reshape(-1)
    # scan: vertex ids in (point, axis) order
    nvert = np.array([bin(m).count("1") for m in range(8)])[mask]
    vbase = np.concatenate([[0], np.cumsum(nvert)[:-1]]) if n else np.zeros(0, np.int64)
    V = int(nvert.sum())
    # emit vertices
    pts, axes = [], []
    for a in range(3):
        p = np.flatnonzero((mask >> a) & 1)
        pts.append(p)
        axes.append(np.full(p.shape, a))
    pts, axes = np.concatenate(pts), np.concatenate(axes)
    order = np.argsort(pts * 3 + axes, kind="stable")
    pts, axes = pts[order], axes[order]
    idx = np.stack(np.unravel_index(pts, vol.shape), axis=1)                 # [V, 3]
    j = pts + np.array(strides)[axes]
    v0, v1 = flat[pts], flat[j]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (level - v0) / (v1 - v0)
    t = np.where(np.isnan(t), np.float32(0.5), np.minimum(np.maximum(t, np.float32(0)), np.float32(1))).astype(np.float32)
    fi = idx.astype(np.float32)
    verts = np.empty((V, 3), dtype=np.float32)
    for b in range(3):
        on = axes == b
        verts[:, b] = np.where(on, org[b] + (fi[:, b] + t) * sp[b], org[b] + fi[:, b] * sp[b])
    nrm = None
    if normals:
        g = _grad(vol, sp).reshape(3, -1)
        g0, g1 = g[:, pts].T, g[:, j].T
        nv = -(g0 + t[:, None] * (g1 - g0))
        ln = np.sqrt(nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1] + nv[:, 2] * nv[:, 2])
        s = np.where(ln > 0, ln, np.float32(1)).astype(np.float32)
        nrm = (nv / s[:, None]).astype(np.float32)
    # emit faces
    cells = np.flatnonzero(NTRI[case] > 0)
    cc = case[cells]
    tris = TRI[cc][:, :15].reshape(-1, 5, 3)
    valid = np.arange(5)[None, :] < NTRI[cc][:, None]
    e = tris[valid].astype(np.int64)                                           # [F, 3] in (cell, table order)
    cell_of = np.repeat(cells, NTRI[cc])
    corner, axis = EDGE_CORNER[e], EDGE_AXIS[e]
    owner = cell_of[:, None] + (corner & 1) * strides[0] + ((corner >> 1) & 1) * strides[1] + ((corner >> 2) & 1) * strides[2]
    rank = np.array([[bin(m & ((1 << a) - 1)).count("1") for a in range(3)] for m in range(8)])
    faces = (vbase[owner] + rank[mask[owner], axis]).astype(np.int32).reshape(-1, 3)
    return verts, faces, nrm


def edge_use(faces):
    """{(a, b): count of the directed edge a -> b} over all triangles"""
    d = {}
    for f in faces:
        for k in range(3):
            key = (int(f[k]), int(f[(k + 1) % 3]))
            d[key] = d.get(key, 0) + 1
    return d


def check_closed_oriented(verts, faces, box_lo=None, box_hi=None, tol=1e-6):
    """every undirected edge is used by exactly 2 triangles, once in each direction — except edges whose two vertices lie on one face of
    the volume's box (box_lo / box_hi per axis), which may be open.  Returns the number of open boundary edges."""
    use = edge_use(faces)
    open_edges = 0
    for (a, b), k in use.items():
        back = use.get((b, a), 0)
        if k == 1 and back == 1:
            continue
        on_box = False
        if box_lo is not None:
            for ax in range(3):
                for bound in (box_lo[ax], box_hi[ax]):
                    if abs(verts[a, ax] - bound) <= tol and abs(verts[b, ax] - bound) <= tol:
                        on_box = True
        assert on_box and k == 1 and back == 0, f"edge {a}->{b}: used {k}x, reverse {back}x"
        open_edges += 1
    return open_edges


def euler_characteristic(verts, faces):
    used = np.unique(faces)
    edges = {tuple(sorted((int(f[k]), int(f[(k + 1) % 3])))) for f in faces for k in range(3)}
    return len(used) - len(edges) + len(faces)


def face_normals(verts, faces):
    v = verts.astype(np.float64)
    return np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])


def read_ply(path):
    """Parser of what customnerf_amd.mesh.write_ply writes (binary little-endian, its properties only) -> dict of NumPy arrays: verts,
    faces, and normals / colors when present."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    elems, cur = [], None
    for ln in lines[2:]:
        p = ln.split()
        if not p or p[0] in ("comment", "end_header"):
            continue
        if p[0] == "element":
            cur = [p[1], int(p[2]), []]
            elems.append(cur)
        elif p[0] == "property":
            cur[2].append(p[1:])
    types = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    out, off = {}, end
    for name, count, props in elems:
        if name == "vertex":
            dt = np.dtype([(q[1], types[q[0]]) for q in props])
            rec = np.frombuffer(data, dtype=dt, count=count, offset=off)
            out["verts"] = np.stack([rec["x"], rec["y"], rec["z"]], 1)
            if "nx" in dt.names:
                out["normals"] = np.stack([rec["nx"], rec["ny"], rec["nz"]], 1)
            if "red" in dt.names:
                out["colors"] = np.stack([rec["red"], rec["green"], rec["blue"]], 1)
        elif name == "face":
            if props != [["list", "uchar", "int", "vertex_indices"]]:
                raise ValueError(f"{path}: unsupported face properties {props}")
            dt = np.dtype([("n", "u1"), ("vertex_indices", "<i4", (3,))])
            rec = np.frombuffer(data, dtype=dt, count=count, offset=off)
            if count and not (rec["n"] == 3).all():
                raise ValueError(f"{path}: only triangles are supported")
            out["faces"] = rec["vertex_indices"].copy()
        else:
            raise ValueError(f"{path}: unexpected element {name}")
        off += dt.itemsize * count
    return out
