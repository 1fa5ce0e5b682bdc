"""NumPy restatement of the texture atlas of csrc/mesh_texture.hip (cnerf_mesh_atlas_*; rules in include/customnerf_hip.h): layout, UVs,
texel owners, texel -> surface point and view direction, all in float32 with the kernels' operation order, so that UVs and points are
bit-equal to the device's."""
import math

import numpy as np

f32 = np.float32


def layout(F, R):
    """(n, s): n = max(1, ceil(sqrt(P))) cells per row, s = floor(R / n); ValueError when R is outside [16, 16384] or s < 4"""
    if R < 16 or R > 16384:
        raise ValueError("resolution")
    P = (F + 1) // 2
    n = max(1, math.isqrt(P - 1) + 1) if P else 1
    s = R // n
    if s < 4:
        raise ValueError("cells smaller than 4 x 4 texels")
    return n, s


def corner_local(s):
    """local texel (i, j) of the corners: [2 faces (A, B)][3 corners][i, j]"""
    return np.array([[(0, 0), (0, s - 2), (s - 2, 0)], [(s - 1, s - 1), (s - 1, 2), (2, s - 1)]], dtype=np.int64)


def corner_texels(F, R):
    """global texel (X, Y) of every face corner, [F, 3, 2] int64"""
    n, s = layout(F, R)
    f = np.arange(F)
    p = f // 2
    cx, cy = p % n, p // n
    loc = corner_local(s)[f % 2]                                           # [F, 3, 2]
    return np.stack([cx[:, None] * s + loc[..., 0], cy[:, None] * s + loc[..., 1]], -1)


def uvs(F, R):
    """[F, 3, 2] float32: u = (X + 0.5) / R, v = 1 - (Y + 0.5) / R"""
    XY = corner_texels(F, R).astype(f32)
    Rf = f32(R)
    u = (XY[..., 0] + f32(0.5)) / Rf
    v = f32(1.0) - (XY[..., 1] + f32(0.5)) / Rf
    return np.stack([u, v], -1).astype(f32)


def owner_map(F, R):
    """[R, R] int64 (row Y, column X): the face that owns each texel, -1 where none does"""
    n, s = layout(F, R)
    P = (F + 1) // 2
    Y, X = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    cx, cy, i, j = X // s, Y // s, X % s, Y % s
    p = cy * n + cx
    f = 2 * p + (i + j > s - 1)
    used = (cx < n) & (cy < n) & (p < P) & (f < F)
    return np.where(used, f, -1)


def cell_texels(F, R, t0=0, t1=None):
    """for cell texels t in [t0, t1): (face or -1 when un-owned, local i, j, global X, Y), int64 arrays"""
    n, s = layout(F, R)
    P = (F + 1) // 2
    t1 = P * s * s if t1 is None else t1
    t = np.arange(t0, t1, dtype=np.int64)
    p, r = t // (s * s), t % (s * s)
    j, i = r // s, r % s
    f = 2 * p + (i + j > s - 1)
    X, Y = (p % n) * s + i, (p // n) * s + j
    return np.where(f < F, f, -1), i, j, X, Y


def _interp(a0, a1, a2, w1, w2, corner):
    o = (a0 + w1[:, None] * (a1 - a0)) + w2[:, None] * (a2 - a0)
    for k, a in enumerate((a0, a1, a2)):
        o = np.where((corner == k)[:, None], a, o)
    return o.astype(f32)


def _look(x):
    """(-x / |x|, ok) with ok where |x|^2 is positive and finite; |x|^2 summed x0^2 + x1^2 + x2^2 in float32"""
    with np.errstate(all="ignore"):
        l2 = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
        ok = (l2 > 0) & np.isfinite(l2)
        l = np.sqrt(np.where(ok, l2, f32(1))).astype(f32)
        return -(x / l[:, None]), ok


def points(verts, faces, R, normals=None, t0=0, t1=None):
    """(x [N, 3], d [N, 3]) float32 of the cell texels t in [t0, t1), as k_atlas_points writes them"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(fc)
    _, s = layout(F, R)
    face, i, j, _, _ = cell_texels(F, R, t0, t1)
    N = len(face)
    x = np.zeros((N, 3), f32)
    d = np.tile(np.array([0, 0, -1], f32), (N, 1))
    own = face >= 0
    fo, i, j = face[own], i[own], j[own]
    b = fo % 2 == 1
    with np.errstate(all="ignore"):
        w1 = np.where(b, (s - 1 - j).astype(f32) / f32(s - 3), j.astype(f32) / f32(s - 2)).astype(f32)
        w2 = np.where(b, (s - 1 - i).astype(f32) / f32(s - 3), i.astype(f32) / f32(s - 2)).astype(f32)
    cl = corner_local(s)[b.astype(np.int64)]                                # [M, 3, 2]
    hit = (cl[..., 0] == i[:, None]) & (cl[..., 1] == j[:, None])          # [M, 3]
    corner = np.where(hit.any(1), hit.argmax(1), -1)
    tri = fc[fo]
    p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    x[own] = _interp(p0, p1, p2, w1, w2, corner)
    ok = np.zeros(len(fo), bool)
    dd = np.zeros((len(fo), 3), f32)
    if normals is not None:
        nv = np.asarray(normals, f32).reshape(-1, 3)
        nn = _interp(nv[tri[:, 0]], nv[tri[:, 1]], nv[tri[:, 2]], w1, w2, corner)
        dd, ok = _look(nn)
    e1, e2 = p1 - p0, p2 - p0
    gn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(f32)
    dg, okg = _look(gn)
    dd = np.where(ok[:, None], dd, np.where(okg[:, None], dg, np.array([0, 0, -1], f32)))
    d[own] = dd
    return x, d.astype(f32)


def bilinear(tex, u, v):
    """bilinear lookup of tex [R, R, C] at UVs (u, v) (arrays), v up, clamp to edge -> [N, C] float64"""
    R = tex.shape[0]
    px = np.asarray(u, np.float64) * R - 0.5
    py = (1.0 - np.asarray(v, np.float64)) * R - 0.5
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    fx, fy = (px - x0)[:, None], (py - y0)[:, None]
    t = tex.astype(np.float64)

    def at(X, Y):
        return t[np.clip(Y, 0, R - 1), np.clip(X, 0, R - 1)]
    return ((1 - fx) * (1 - fy) * at(x0, y0) + fx * (1 - fy) * at(x0 + 1, y0) + (1 - fx) * fy * at(x0, y0 + 1)
            + fx * fy * at(x0 + 1, y0 + 1))


def read_png(path):
    """decode an 8-bit RGB, non-interlaced PNG with filter 0 rows (what mesh.write_png writes) -> [H, W, 3] uint8"""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        ln, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + ln]
        crc, = struct.unpack(">I", data[pos + 8 + ln:pos + 12 + ln])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, tag
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + ln
    W, H, depth, ctype, comp, filt, lace = hdr
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, 3).copy()


def read_obj(path):
    """the v / vt / vn / f lines of an OBJ -> dict(verts [V, 3], uvs [T, 2], normals [N, 3] float32, f [F, 3, k] int64 (1-based), mtllib)"""
    v, vt, vn, f, mtl = [], [], [], [], None
    for line in open(path):
        w = line.split()
        if not w:
            continue
        if w[0] == "v":
            v.append([float(a) for a in w[1:4]])
        elif w[0] == "vt":
            vt.append([float(a) for a in w[1:3]])
        elif w[0] == "vn":
            vn.append([float(a) for a in w[1:4]])
        elif w[0] == "f":
            f.append([[int(b) if b else 0 for b in a.split("/")] for a in w[1:]])
        elif w[0] == "mtllib":
            mtl = w[1]
    return dict(verts=np.array(v, f32).reshape(-1, 3), uvs=np.array(vt, f32).reshape(-1, 2), normals=np.array(vn, f32).reshape(-1, 3),
                f=np.array(f, np.int64).reshape(len(f), 3, -1) if f else np.zeros((0, 3, 1), np.int64), mtllib=mtl)
