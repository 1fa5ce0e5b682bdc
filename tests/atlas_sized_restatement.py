"""NumPy restatement of the area-proportional texture atlas of csrc/mesh_texture.hip (cnerf_mesh_atlas_sized_*; rules in
include/customnerf_hip.h): size keys, the threshold e, classes, ranks, cells on the Z-order curve, UVs, texel owners and
texel -> surface point and view direction, in float32 with the kernels' operation order, so that keys, cells, UVs and points are bit-equal
to the device's.  Inside a cell the rules are those of tests/atlas_restatement.py, used here with the cell's own s."""
import math

import numpy as np

import atlas_restatement as A

f32 = np.float32
BINS = 2048


def classes_of(R):
    """K = min(7, log2(R) - 2); ValueError unless R is a power of two in [16, 16384]"""
    R = int(R)
    if R < 16 or R > 16384 or R & (R - 1):
        raise ValueError("resolution must be a power of two in [16, 16384]")
    return min(7, R.bit_length() - 3)


def size_keys(verts, faces):
    """[F] int64: float_bits(L2) >> 20 with L2 the longest squared edge, (dx dx + dy dy) + dz dz in float32; 0 unless L2 is finite and > 0"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    if not len(fc):
        return np.zeros(0, np.int64), np.zeros(0, f32)
    with np.errstate(all="ignore"):
        ls = []
        for a, b in ((0, 1), (1, 2), (2, 0)):
            d = v[fc[:, b]] - v[fc[:, a]]
            ls.append((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        L2 = np.fmax(np.fmax(ls[0], ls[1]), ls[2]).astype(f32)               # a NaN beside a number is ignored
        ok = np.isfinite(L2) & (L2 > 0)
    return np.where(ok, L2.view(np.uint32).astype(np.int64) >> 20, 0), L2


def histogram(keys):
    return np.bincount(np.asarray(keys, np.int64), minlength=BINS).astype(np.int64)


def class_of(keys, e, K):
    keys = np.asarray(keys, np.int64)
    return np.where(keys < e, 0, np.minimum((keys - e) >> 4, K))


def class_counts(hist, e, K):
    """n_k, [8] int64 (0 above K), from the key histogram"""
    return np.bincount(class_of(np.arange(BINS), e, K), weights=np.asarray(hist, np.float64), minlength=8).astype(np.int64)   # exact: < 2^53


def tiles_of(n):
    return int(sum(((int(c) + 1) // 2) * 4 ** k for k, c in enumerate(n)))


def layout(hist, R):
    """(e, n [8], tiles): e the smallest threshold in [0, 2048] with tiles(e) <= (R / 4)^2; ValueError when none fits"""
    K = classes_of(R)
    cap = (R // 4) ** 2
    for e in range(BINS + 1):
        n = class_counts(hist, e, K)
        t = tiles_of(n)
        if t <= cap:
            return e, n, t
    raise ValueError("cells smaller than 4 x 4 texels")


def threshold(e):
    """the edge length e stands for: sqrt of the float32 with bits e << 20"""
    return math.inf if e >= 2040 else math.sqrt(float(np.array([e << 20], np.uint32).view(f32)[0]))


def even_bits(o):
    o = np.asarray(o, np.int64)
    x = np.zeros_like(o)
    for b in range(16):
        x |= ((o >> (2 * b)) & 1) << b
    return x


def interleave(tx, ty):
    tx, ty = np.asarray(tx, np.int64), np.asarray(ty, np.int64)
    o = np.zeros_like(tx)
    for b in range(16):
        o |= (((tx >> b) & 1) << (2 * b)) | (((ty >> b) & 1) << (2 * b + 1))
    return o


class Plan:
    pass


def plan(verts, faces, R, e=None):
    """The whole plan of a mesh: e, K, counts n [8], class offsets O [8] (tiles) and B [8] (cells), tiles, texels, per face k, rank, and
    cells [F, 4] = (X0, Y0, s, b); owner [cells, 2] = (face A, face B or -1).  `e` overrides the threshold (any value whose tiles fit)."""
    p = Plan()
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(fc)
    p.R, p.F, p.K = int(R), F, classes_of(R)
    p.keys, p.L2 = size_keys(verts, fc)
    p.hist = histogram(p.keys)
    p.e, p.n, p.tiles = layout(p.hist, R)
    if e is not None:
        p.e, p.n = e, class_counts(p.hist, e, p.K)
        p.tiles = tiles_of(p.n)
        assert p.tiles <= (R // 4) ** 2
    p.texels = 16 * p.tiles
    C = (p.n + 1) // 2
    p.O, p.B = np.zeros(8, np.int64), np.zeros(8, np.int64)
    o = b = 0
    for k in range(7, -1, -1):
        p.O[k], p.B[k] = o, b
        o += C[k] * 4 ** k
        b += C[k]
    p.ncells = b
    p.k = class_of(p.keys, p.e, p.K)
    p.rank = np.zeros(F, np.int64)
    for k in range(8):
        m = p.k == k
        p.rank[m] = np.arange(m.sum())
    c, bb = p.rank >> 1, p.rank & 1
    o = p.O[p.k] + c * 4 ** p.k
    p.cells = np.stack([4 * even_bits(o), 4 * even_bits(o >> 1), 4 << p.k, bb], -1).astype(np.int32).reshape(F, 4)
    p.owner = np.full((p.ncells, 2), -1, np.int64)
    p.owner[p.B[p.k] + c, bb] = np.arange(F)
    return p


def _corner_ij(s, b):
    """local texel (i, j) of the three corners for arrays s, b -> [N, 3, 2] int64 (A.corner_local with a per-row s)"""
    out = np.zeros((len(s), 3, 2), np.int64)
    for ss in np.unique(s):
        m = s == ss
        out[m] = A.corner_local(int(ss))[b[m]]
    return out


def corner_texels(p):
    """global texel (X, Y) of every face corner, [F, 3, 2] int64"""
    c = p.cells.astype(np.int64)
    return c[:, None, :2] + _corner_ij(c[:, 2], c[:, 3])


def uvs(p):
    XY = corner_texels(p).astype(f32)
    Rf = f32(p.R)
    u = (XY[..., 0] + f32(0.5)) / Rf
    v = f32(1.0) - (XY[..., 1] + f32(0.5)) / Rf
    return np.stack([u, v], -1).astype(f32).reshape(p.F, 3, 2)


def cell_texels(p, t0=0, t1=None):
    """for cell texels t in [t0, t1): (face or -1 when un-owned, local i, j, global X, Y, cell edge s), int64 arrays"""
    t = np.arange(t0, p.texels if t1 is None else t1, dtype=np.int64)
    tile = t >> 4
    k = np.zeros(len(t), np.int64)
    for q in range(1, 8):                                                     # O descends with k
        k = np.where(tile < p.O[q - 1], q, k)
    rel = t - 16 * p.O[k]
    s = 4 << k
    c, r = rel // (s * s), rel % (s * s)
    j, i = r // s, r % s
    b = (i + j > s - 1).astype(np.int64)
    o = p.O[k] + c * 4 ** k
    face = p.owner[p.B[k] + c, b] if len(t) else np.zeros(0, np.int64)
    return face, i, j, 4 * even_bits(o) + i, 4 * even_bits(o >> 1) + j, s


def owner_map(p):
    """[R, R] int64 (row Y, column X): the face that owns each texel, -1 where none does — from the cells, not from the texel order"""
    own = np.full((p.R, p.R), -1, np.int64)
    c = p.cells.astype(np.int64)
    for f in range(p.F):
        X0, Y0, s, b = c[f]
        j, i = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
        m = (i + j > s - 1) == bool(b)
        assert (own[Y0 + j[m], X0 + i[m]] == -1).all()
        own[Y0 + j[m], X0 + i[m]] = f
    return own


def in_cells(p):
    """[R, R] bool: the fill predicate's complement, interleave(X >> 2, Y >> 2) < tiles"""
    Y, X = np.meshgrid(np.arange(p.R), np.arange(p.R), indexing="ij")
    return interleave(X >> 2, Y >> 2) < p.tiles


def points(p, verts, faces, normals=None, t0=0, t1=None):
    """(x [N, 3], d [N, 3]) float32 of the cell texels t in [t0, t1), as k_sized_points writes them"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    face, i, j, _, _, s = cell_texels(p, t0, t1)
    N = len(face)
    x = np.zeros((N, 3), f32)
    d = np.tile(np.array([0, 0, -1], f32), (N, 1))
    own = face >= 0
    fo, i, j, s = face[own], i[own], j[own], s[own]
    b = i + j > s - 1
    sf = s.astype(f32)
    with np.errstate(all="ignore"):
        w1 = np.where(b, (s - 1 - j).astype(f32) / (sf - f32(3)), j.astype(f32) / (sf - f32(2))).astype(f32)
        w2 = np.where(b, (s - 1 - i).astype(f32) / (sf - f32(3)), i.astype(f32) / (sf - f32(2))).astype(f32)
    cl = _corner_ij(s, b.astype(np.int64))
    hit = (cl[..., 0] == i[:, None]) & (cl[..., 1] == j[:, None])
    corner = np.where(hit.any(1), hit.argmax(1), -1)
    tri = fc[fo]
    p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    with np.errstate(all="ignore"):
        x[own] = A._interp(p0, p1, p2, w1, w2, corner)
        ok = np.zeros(len(fo), bool)
        dd = np.zeros((len(fo), 3), f32)
        if normals is not None:
            nv = np.asarray(normals, f32).reshape(-1, 3)
            nn = A._interp(nv[tri[:, 0]], nv[tri[:, 1]], nv[tri[:, 2]], w1, w2, corner)
            dd, ok = A._look(nn)
        e1, e2 = p1 - p0, p2 - p0
        gn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(f32)
        dg, okg = A._look(gn)
    dd = np.where(ok[:, None], dd, np.where(okg[:, None], dg, np.array([0, 0, -1], f32)))
    d[own] = dd
    return x, d.astype(f32)
