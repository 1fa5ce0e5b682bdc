"""NumPy restatement of the welded vertices, tangent frames and tangent-space normal maps (csrc/mesh_tangent.hip, k_bake_tspace of
csrc/mesh_bake.h), written from the rules in include/customnerf_hip.h (cnerf_mesh_tangent_*): the weld on the bit patterns of the UVs, the
frames in float64 with one rounding per written operation and sums in ascending corner index, the per-texel code in float32.  Integers are
equal to the device's and floats bit-equal."""
import numpy as np

import atlas_proj_restatement as AP
import atlas_restatement as A
import atlas_sized_restatement as AS

f32, f64 = np.float32, np.float64
DBL_MIN, FLT_MIN = np.finfo(f64).tiny, np.finfo(f32).tiny


# ---------------------------------------------------------------------------------------------------------------- 1a. weld
def weld(faces, uvs):
    """(corner_vertex [F, 3] int64, vertex_corner [W] int64).  Corner c = 3 f + k has the key (vertex, bits of u, bits of v); equal keys are
    one output vertex; output vertices are numbered by ascending vertex, then by ascending smallest corner of the group."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    bits = np.ascontiguousarray(np.asarray(uvs, f32).reshape(-1, 2)).view(np.uint32)
    leader = {}
    key_of = []
    for c, v in enumerate(f.reshape(-1).tolist()):                             # ascending corner: the first of a key is its smallest
        key = (v, int(bits[c, 0]), int(bits[c, 1]))
        leader.setdefault(key, c)
        key_of.append(key)
    order = sorted(leader.items(), key=lambda kv: (kv[0][0], kv[1]))           # by vertex, then by smallest corner
    rank = {key: i for i, (key, _) in enumerate(order)}
    cv = np.array([rank[k] for k in key_of], np.int64).reshape(-1, 3)
    return cv, np.array([c for _, c in order], np.int64)


# ---------------------------------------------------------------------------------------------------------------- 1b. frames
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _pos(x):
    return (x > 0) & (x < np.inf)


def face_terms(verts, faces, uvs):
    """(ok [F], cT [F, 3], cB [F, 3], cN [F, 3], det [F]) float64: what a face gives the groups of its corners"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    uv = np.asarray(uvs, f32).reshape(-1, 3, 2)
    with np.errstate(all="ignore"):
        p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        e1, e2 = (p1 - p0).astype(f32).astype(f64), (p2 - p0).astype(f32).astype(f64)      # float32 differences, then float64
        d1, d2 = (uv[:, 1] - uv[:, 0]).astype(f32).astype(f64), (uv[:, 2] - uv[:, 0]).astype(f32).astype(f64)
        du1, dv1, du2, dv2 = d1[:, 0], d1[:, 1], d2[:, 0], d2[:, 1]
        det = du1 * dv2 - du2 * dv1
        s = np.where(det < 0, -1.0, 1.0)
        T = s[:, None] * (e1 * dv2[:, None] - e2 * dv1[:, None])
        B = s[:, None] * (e2 * du1[:, None] - e1 * du2[:, None])
        c = _cross(e1, e2)
        A2, lT, lB = np.sqrt(_dot(c, c)), np.sqrt(_dot(T, T)), np.sqrt(_dot(B, B))
        ok = (det != 0) & np.isfinite(det) & _pos(A2) & _pos(lT) & _pos(lB)
        cT = (A2[:, None] * T) / lT[:, None]
        cB = (A2[:, None] * B) / lB[:, None]
    return ok, cT, cB, c, det


def _fallback(n):
    """c - n n_a for the unit axis a of the smallest |n_a|, the lowest on ties"""
    a = np.argmin(np.abs(n), -1)
    c = np.zeros_like(n)
    c[np.arange(len(n)), a] = 1
    return c - n * n[np.arange(len(n)), a][:, None]


def frames(verts, faces, uvs, normals=None, welded=None):
    """(tangents [F, 3, 4] float32, group normals [W, 3] float32, corner_vertex, vertex_corner)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    cv, vc = weld(f, uvs) if welded is None else welded
    W = len(vc)
    ok, cT, cB, cN, _ = face_terms(verts, f, uvs)
    ST, SB, SN = np.zeros((W, 3), f64), np.zeros((W, 3), f64), np.zeros((W, 3), f64)
    flat = cv.reshape(-1)
    for c in range(3 * F):                                                     # every sum in ascending corner index
        if ok[c // 3]:
            g = flat[c]
            ST[g] += cT[c // 3]
            SB[g] += cB[c // 3]
            SN[g] += cN[c // 3]
    gv = f.reshape(-1)[vc] if W else np.zeros(0, np.int64)                     # the vertex of every group
    with np.errstate(all="ignore"):
        n = np.asarray(normals, f32).reshape(-1, 3)[gv].astype(f64) if normals is not None else SN.copy()
        q = _dot(n, n)
        n = np.where(_pos(q)[:, None], n / np.sqrt(q)[:, None], 0.0)
        t = ST - n * _dot(n, ST)[:, None]
        q = _dot(t, t)
        bad = ~((q >= DBL_MIN) & (q < np.inf))
        t = np.where(bad[:, None], _fallback(n), t)
        q = _dot(t, t)
        unit = (t / np.sqrt(q)[:, None]).astype(f32)
        w = np.where(_dot(_cross(n, t), SB) < 0, f32(-1), f32(1)).astype(f32)
    frame = np.concatenate([unit, w[:, None]], 1).astype(f32)
    return frame[flat].reshape(F, 3, 4), n.astype(f32), cv, vc


# ---------------------------------------------------------------------------------------------------------------- 1d. vertex buffers
def vertices(verts, faces, uvs, normals=None):
    """the arrays of a glTF primitive: positions, normals, uvs (u, 1 - v), tangents, indices"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    uv = np.asarray(uvs, f32).reshape(-1, 2)
    tan, gn, cv, vc = frames(v, f, uvs, normals)
    gv = f.reshape(-1)[vc] if len(vc) else np.zeros(0, np.int64)
    nrm = np.asarray(normals, f32).reshape(-1, 3)[gv] if normals is not None else gn
    return {'positions': v[gv], 'normals': nrm.astype(f32), 'uvs': np.stack([uv[vc, 0], f32(1) - uv[vc, 1]], -1).astype(f32),
            'tangents': tan.reshape(-1, 4)[vc], 'indices': cv.astype(np.uint32)}


# ---------------------------------------------------------------------------------------------------------------- 1c. per-texel code
def _cell_weights(face, i, j, s):
    """(w1, w2, corner) float32 of owned cell texels of the uniform and the area layout; s scalar or per texel"""
    s = np.broadcast_to(np.asarray(s, np.int64), face.shape)
    b = i + j > s - 1
    sf = s.astype(f32)
    with np.errstate(all="ignore"):
        w1 = np.where(b, (s - 1 - j).astype(f32) / (sf - f32(3)), j.astype(f32) / (sf - f32(2))).astype(f32)
        w2 = np.where(b, (s - 1 - i).astype(f32) / (sf - f32(3)), i.astype(f32) / (sf - f32(2))).astype(f32)
    cl = AS._corner_ij(s, b.astype(np.int64))
    hit = (cl[..., 0] == i[:, None]) & (cl[..., 1] == j[:, None])
    return w1, w2, np.where(hit.any(1), hit.argmax(1), -1)


def texels(layout, plan, verts, faces, R, normals=None, t0=0, t1=None):
    """For the cell texels [t0, t1) of layout 'uniform' (plan: None), 'area' (plan of atlas_sized_restatement) or 'projected' (plan of
    atlas_proj_restatement): (face [N] (-1: un-owned), w1, w2 float32, corner, flat bool, N [N, 3] = -d of the points pass, X, Y)"""
    F = len(np.asarray(faces).reshape(-1, 3))
    if layout == 'projected':
        t1 = plan.total if t1 is None else t1
        X, Y = plan.X[t0:t1], plan.Y[t0:t1]
        face = plan.owner[Y, X]
        s = plan.snap[face]
        x, y = s[..., 0], s[..., 1]
        px, py = 256 * X + 128, 256 * Y + 128
        A2 = AP._area2(s)
        E = {}
        for k in (1, 2):
            a, b = (k + 1) % 3, (k + 2) % 3
            E[k] = (y[:, b] - y[:, a]) * (px - x[:, a]) - (x[:, b] - x[:, a]) * (py - y[:, a])
        pos = A2 > 0
        Ad = np.where(pos, A2, 1).astype(f64)
        w1 = np.where(pos, (E[1].astype(f64) / Ad).astype(f32), f32(0)).astype(f32)
        w2 = np.where(pos, (E[2].astype(f64) / Ad).astype(f32), f32(0)).astype(f32)
        d = AP.points(plan, verts, faces, normals, t0, t1)[1]
        return face, w1, w2, np.full(len(face), -1), ~pos, -d, X, Y
    if layout == 'uniform':
        _, s = A.layout(F, R)
        face, i, j, X, Y = A.cell_texels(F, R, t0, t1)
        d = A.points(verts, faces, R, normals, t0, face.shape[0] + t0)[1]
    else:
        face, i, j, X, Y, s = AS.cell_texels(plan, t0, t1)
        d = AS.points(plan, verts, faces, normals, t0, face.shape[0] + t0)[1]
    own = face >= 0
    w1, w2, corner = np.zeros(len(face), f32), np.zeros(len(face), f32), np.full(len(face), -1)
    w1[own], w2[own], corner[own] = _cell_weights(face[own], i[own], j[own], s if np.ndim(s) == 0 else s[own])
    return face, w1, w2, corner, np.zeros(len(face), bool), -d, X, Y


def texel_frames(tangents, face, w1, w2, corner, flat, N):
    """(t, B) float32 [M, 3] of owned texels (face >= 0 everywhere): the frame the code is written in"""
    T = np.asarray(tangents, f32).reshape(-1, 3, 4)[face]
    N = N.astype(f32)
    with np.errstate(all="ignore"):
        Ti = A._interp(T[:, 0, :3], T[:, 1, :3], T[:, 2, :3], w1, w2, corner)
        t = (Ti - N * _dot(N, Ti)[:, None]).astype(f32)
        q = _dot(t, t)
        bad = ~((q >= FLT_MIN) & (q < np.inf))
        t = np.where(bad[:, None], _fallback(N), t).astype(f32)
        q = _dot(t, t)
        t = (t / np.sqrt(q)[:, None]).astype(f32)
        b0 = (f32(1) - w1) - w2
        sel = np.zeros(len(face), np.int64)
        best = b0.copy()
        m1 = w1 > best
        sel[m1], best[m1] = 1, w1[m1]
        sel[w2 > best] = 2
        sel = np.where(corner >= 0, corner, sel)
        sel = np.where(flat, 0, sel)
        w = T[np.arange(len(face)), sel, 3]
        B = (w[:, None] * _cross(N, t)).astype(f32)
    assert t.dtype == f32 and B.dtype == f32
    return t, B


def tspace(tangents, face, w1, w2, corner, flat, N, m=None):
    """rgb float32 [N, 3] as k_bake_tspace writes it; m [N, 3] float32 or None (the texel's own normal: (0.5, 0.5, 1) exactly)"""
    rgb = np.tile(np.array([0.5, 0.5, 1.0], f32), (len(face), 1))
    own = face >= 0
    if m is None or not own.any():
        return rgb
    Nn = N[own].astype(f32)
    t, B = texel_frames(tangents, face[own], w1[own], w2[own], corner[own], flat[own], Nn)
    mm = np.asarray(m, f32)[own]
    with np.errstate(all="ignore"):
        rgb[own] = np.stack([f32(0.5) + f32(0.5) * _dot(mm, t), f32(0.5) + f32(0.5) * _dot(mm, B), f32(0.5) + f32(0.5) * _dot(mm, Nn)], -1)
    return rgb.astype(f32)


def store_u8(v):
    """round(clamp(v, 0, 1) * 255), half to even, NaN -> 0, as k_bake_store"""
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(np.asarray(v, f32), f32(0)), f32(1))
        return np.rint(c * f32(255)).astype(np.uint8)


def decode(rgb8, t, B, N):
    """the object-space vector a tangent-space byte triple stands for in the frame (t, B, N), float64, not normalised"""
    c = rgb8.astype(f64) / 255.0 * 2.0 - 1.0
    return c[:, 0:1] * t.astype(f64) + c[:, 1:2] * B.astype(f64) + c[:, 2:3] * N.astype(f64)
