"""NumPy restatement of the winding-number rules of csrc/mesh_bvh.hip (include/customnerf_hip.h, cnerf_mesh_winding_* and
cnerf_mesh_bvh_signed_distance).  Three things:
  exact(...)        the reference: the brute-force sum of the Van Oosterom-Strackee solid angles over the faces that take part, in float64;
  tree / moments    the build's order of the records (Morton codes of the centroids, then the face index) and the per-node moments, float32
                    with one rounding per written operation: what the device buffer must equal bit for bit;
  walk(...)         the depth-first walk with the dipole far field: the accept decisions and every term's arithmetic in `dtype` in the
                    order written (float32: the device's decisions and terms, but for atan2, which is taken in float64 of the float32
                    numerator and denominator), each query's terms summed in its own traversal order, in float64.
A plain module, NumPy only."""
import numpy as np

from bvh_restatement import participating

F32 = np.float32
LEAF = 4
FOURPI32 = F32(12.566370614359172)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _len(u):
    return np.sqrt(_dot(u, u))


def solid_angles(q, a, b, c, dtype=np.float64):
    """Omega / 4 pi of the triangles (a, b, c: [F, 3]) seen from the points q [Q, 3] -> [Q, F] float64; the numerator and denominator are
    computed in `dtype` by the header's rule, the arctangent in float64"""
    q, a, b, c = (np.asarray(t, dtype) for t in (q, a, b, c))
    a, b, c = (t[None] - q[:, None] for t in (a, b, c))
    with np.errstate(all='ignore'):
        num = _dot(a, _cross(b, c))
        la, lb, lc = _len(a), _len(b), _len(c)
        den = (((la * lb) * lc + _dot(a, b) * lc) + _dot(b, c) * la) + _dot(c, a) * lb
        t = 2.0 * np.arctan2(num.astype(np.float64), den.astype(np.float64)) / (4.0 * np.pi)
    return np.where(num == 0, 0.0, t)


def exact(verts, faces, points, block=256):
    """the reference: w [Q] float64, the sum over the faces that take part; 0 for a non-finite point"""
    ok, _ = participating(verts, faces)
    f = np.asarray(faces, np.int64).reshape(-1, 3)[ok]
    v = np.asarray(verts, F32).reshape(-1, 3)
    q = np.asarray(points, F32).reshape(-1, 3)
    fin = np.isfinite(q).all(1)
    w = np.zeros(len(q))
    if len(f):
        a, b, c = (v[f[:, k]] for k in range(3))
        rows = np.nonzero(fin)[0]
        for s in range(0, len(rows), block):
            r = rows[s:s + block]
            w[r] = solid_angles(q[r], a, b, c).sum(1)
    return w


# ------------------------------------------------------------------------------------------------ the build's order and shape
def _spread(v):
    v = v.astype(np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000ff)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300f00f)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030c30c3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def tree(verts, faces):
    """-> dict: order [n] (the faces that take part in the build's sorted order), rec [LEAF NL, 3, 3] float32 (their vertices, NaN for the
    padding), valid [LEAF NL], NL, D"""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ok, _ = participating(verts, faces)
    idx = np.nonzero(ok)[0]
    n = len(idx)
    NL = (n + LEAF - 1) // LEAF
    D = 0 if NL <= 1 else int(NL - 1).bit_length()
    rec = np.full((LEAF * NL, 3, 3), np.nan, F32)
    valid = np.zeros(LEAF * NL, bool)
    order = idx
    if n:
        tri = verts[faces[idx]]                                                     # [n, 3, 3]
        cen = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / F32(3.0)
        lo, hi = cen.min(0), cen.max(0)
        with np.errstate(all='ignore'):
            t = ((cen - lo) / (hi - lo)) * F32(1024.0)
        qz = np.where(t >= 0, np.minimum(t, F32(1023.0)), F32(0.0)).astype(np.uint32)    # NaN (a flat box) -> 0
        code = _spread(qz[:, 0]) | (_spread(qz[:, 1]) << np.uint32(1)) | (_spread(qz[:, 2]) << np.uint32(2))
        perm = np.lexsort((idx, code))
        order = idx[perm]
        rec[:n] = tri[perm]
        valid[:n] = True
    return {'order': order, 'rec': rec, 'valid': valid, 'NL': NL, 'D': D, 'n': n}


def _leaf_range(j, NL, D):
    return (j * NL) >> D, ((j + 1) * NL) >> D


def moments(tr):
    """the moments buffer as float32 [2^(D + 1), 2, 4]: [i, 0] = (p, r), [i, 1] = (N, A); row 0 is unused (zeros)"""
    NL, D, rec, valid = tr['NL'], tr['D'], tr['rec'], tr['valid']
    mom = np.zeros((2 << D, 2, 4), F32)
    zero, half, third = F32(0.0), F32(0.5), F32(3.0)
    with np.errstate(all='ignore'):
        for j in range(1 << D):
            l0, l1 = _leaf_range(j, NL, D)
            A, N, S, M, cnt = zero, np.zeros(3, F32), np.zeros(3, F32), np.zeros(3, F32), 0
            slots = [l0 * LEAF + t for t in range(LEAF) if l0 < l1 and valid[l0 * LEAF + t]]
            for s in slots:
                a, b, c = rec[s]
                x = _cross(b - a, c - a)
                Ai = half * _len(x)
                A = A + Ai
                ci = ((a + b) + c) / third
                N = N + half * x
                S = S + Ai * ci
                M = M + ci
                cnt += 1
            p, r = np.zeros(3, F32), F32(-1.0)
            if cnt:
                p = M / F32(cnt) if A == 0 else S / A
                r = zero
                for s in slots:
                    for vtx in rec[s]:
                        r = np.maximum(r, _len(vtx - p))
            i = (1 << D) + j
            mom[i, 0, :3], mom[i, 0, 3], mom[i, 1, :3], mom[i, 1, 3] = p, r, N, A
        for d in range(D - 1, -1, -1):
            i = np.arange(1 << d, 2 << d)
            L, R = mom[2 * i], mom[2 * i + 1]
            A = L[:, 1, 3] + R[:, 1, 3]
            pl, pr = L[:, 0, :3], R[:, 0, :3]
            p = np.where((A == 0)[:, None], half * (pl + pr), (L[:, 1, 3:] * pl + R[:, 1, 3:] * pr) / A[:, None])
            r = np.maximum(_len(p - pl) + L[:, 0, 3], _len(p - pr) + R[:, 0, 3])
            out = np.zeros((len(i), 2, 4), F32)
            out[:, 0, :3], out[:, 0, 3], out[:, 1, :3], out[:, 1, 3] = p, r, L[:, 1, :3] + R[:, 1, :3], A
            el, er = L[:, 0, 3] < 0, R[:, 0, 3] < 0
            out[er] = L[er]
            out[el] = R[el]
            mom[i] = out
    return mom


# ------------------------------------------------------------------------------------------------ the walk
def walk(tr, mom, points, beta=2.0, dtype=F32):
    """-> (w [Q] float64, accepted [Q], triangles [Q]): the walk of the header for every point, decisions and terms in `dtype`"""
    NL, D, rec, valid = tr['NL'], tr['D'], tr['rec'], tr['valid']
    q = np.asarray(points, F32).reshape(-1, 3)
    Q = len(q)
    w, acc, tri = np.zeros(Q), np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    if not tr['n']:
        return w, acc, tri
    qd = q.astype(dtype)
    m = mom.astype(dtype)
    beta2 = dtype(F32(beta)) * dtype(F32(beta))
    fourpi = dtype(FOURPI32)

    def visit(node, depth, rows):
        if not len(rows) or m[node, 0, 3] < 0:
            return
        with np.errstate(all='ignore'):
            d = m[node, 0, :3][None] - qd[rows]
            d2 = _dot(d, d)
            far = d2 > beta2 * (m[node, 0, 3] * m[node, 0, 3])
            if far.any():
                term = _dot(m[node, 1, :3][None], d[far]) / (fourpi * (d2[far] * np.sqrt(d2[far])))
                w[rows[far]] += term.astype(np.float64)
                acc[rows[far]] += 1
        near = rows[~far]
        if not len(near):
            return
        if depth == D:
            l0, l1 = _leaf_range(node - (1 << D), NL, D)
            for t in range(LEAF if l0 < l1 else 0):
                s = l0 * LEAF + t
                if valid[s]:
                    w[near] += solid_angles(q[near], rec[s, 0][None], rec[s, 1][None], rec[s, 2][None], dtype)[:, 0]
                    tri[near] += 1
        else:
            visit(2 * node, depth + 1, near)
            visit(2 * node + 1, depth + 1, near)

    visit(1, 0, np.nonzero(np.isfinite(q).all(1))[0])
    return w, acc, tri
