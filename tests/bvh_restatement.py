"""NumPy restatement of csrc/mesh_bvh.hip's rules (include/customnerf_hip.h, cnerf_mesh_bvh_* / cnerf_mesh_sample_*), float32 with one rounding
per written operation, vectorised over the faces: the point-triangle rule with the regions as masks in the header's order, the brute-force
closest face (smallest index on a tie, NaN never wins), the surface sampler and mesh.distance() on top of them.  No tree here: the
definition of the result does not mention one.  closest64 is the same rule in float64 for cross-checks."""
import math

import numpy as np

F32 = np.float32
MAX_K = 256


def participating(verts, faces):
    """mask [F] of the faces that take part, and the flags (bit 0 bad index, bit 1 non-finite)"""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(verts)
    inr = ((faces >= 0) & (faces < V)).all(1)
    fin = np.zeros(len(faces), bool)
    fin[inr] = np.isfinite(verts[faces[inr]]).all((1, 2))
    return inr & fin, (0 if inr.all() else 1) | (2 if (inr & ~fin).any() else 0)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def point_triangles(p, a, b, c, dtype=F32):
    """closest point of each triangle (a, b, c: [F, 3]) to the point p [3] -> (d2 [F], x [F, 3], bary [F, 3]) in `dtype`"""
    one = dtype(1.0)
    p, a, b, c = (np.asarray(t, dtype) for t in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        z, o = np.zeros_like(d1), np.ones_like(d1)
        v3 = d1 / (d1 - d3)
        w5 = d2 / (d2 - d6)
        w6 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        e = one / ((va + vb) + vc)
        v7, w7 = vb * e, vc * e
        regions = [
            (((d1 <= 0) & (d2 <= 0)), a, (o, z, z)),
            (((d3 >= 0) & (d4 <= d3)), b, (z, o, z)),
            (((vc <= 0) & (d1 >= 0) & (d3 <= 0)), a + v3[:, None] * ab, (one - v3, v3, z)),
            (((d6 >= 0) & (d5 <= d6)), c, (z, z, o)),
            (((vb <= 0) & (d2 >= 0) & (d6 <= 0)), a + w5[:, None] * ac, (one - w5, z, w5)),
            (((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)), b + w6[:, None] * (c - b), (z, one - w6, w6)),
            (np.ones(len(a), bool), (a + ab * v7[:, None]) + ac * w7[:, None], ((one - v7) - w7, v7, w7)),
        ]
        x, bary, done = np.zeros_like(a), np.zeros_like(a), np.zeros(len(a), bool)
        for mask, xr, br in regions:
            take = mask & ~done
            x[take] = xr[take]
            bary[take] = np.stack(br, 1)[take]
            done |= take
        r = p - x
        return (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2], x, bary


def closest(verts, faces, points, dtype=F32):
    """brute force -> dict dist2 [Q], face [Q] (int32, -1: none), point [Q, 3], bary [Q, 3]"""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    points = np.asarray(points, F32).reshape(-1, 3)
    ok, _ = participating(verts, faces)
    idx = np.nonzero(ok)[0]
    a, b, c = (verts[faces[idx, k]] for k in range(3))
    Q = len(points)
    out = {'dist2': np.full(Q, np.inf, dtype), 'face': np.full(Q, -1, np.int32), 'point': np.zeros((Q, 3), dtype), 'bary': np.zeros((Q, 3), dtype)}
    if not len(idx):
        return out
    for q in range(Q):
        if not np.isfinite(points[q]).all():
            continue
        d2, x, bary = point_triangles(points[q], a, b, c, dtype)
        if np.isnan(d2).all():
            continue
        m = np.nanmin(d2)
        j = int(np.nonzero(d2 == m)[0][0])                                      # idx is increasing: the smallest face index
        out['dist2'][q], out['face'][q], out['point'][q], out['bary'][q] = m, idx[j], x[j], bary[j]
    return out


def closest64(verts, faces, points):
    return closest(verts, faces, points, np.float64)


def face_orders(verts, faces, spacing):
    """(mask of the faces that take part, area [F] float32, k [F], flags with bit 2 = clamped)"""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ok, flags = participating(verts, faces)
    area, k = np.zeros(len(faces), F32), np.zeros(len(faces), np.int64)
    with np.errstate(all="ignore"):
        v0, v1, v2 = (verts[faces[ok, j]] for j in range(3))
        e1, e2 = v1 - v0, v2 - v0
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        A = F32(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)
        r = np.ceil(np.sqrt(F32(2.0) * A) / F32(spacing))
        clamped = r > MAX_K
        kk = np.where(clamped, MAX_K, np.where(r >= 1, r, 1)).astype(np.int64)   # NaN -> 1
    area[ok], k[ok] = A, kk
    return ok, area, k, flags | (4 if clamped.any() else 0)


def sample(verts, faces, spacing):
    """-> dict points [n, 3], face [n], bary [n, 3], weight [n], total, flags"""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ok, area, k, flags = face_orders(verts, faces, spacing)
    n = k * k
    f = np.repeat(np.arange(len(faces)), n)
    m = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    kk = k[f]
    t = kk * kk - m
    r = np.floor(np.sqrt(t.astype(np.float64))).astype(np.int64)
    r += r * r < t
    i = kk - r
    rem = m - i * (2 * kk - i)
    up, j = rem & 1, rem >> 1
    with np.errstate(all="ignore"):
        den = (3 * kk).astype(F32)
        u, v = (3 * i + 1 + up).astype(F32) / den, (3 * j + 1 + up).astype(F32) / den
        b0 = (F32(1.0) - u) - v
        v0, v1, v2 = (verts[faces[f, c]] for c in range(3))
        pts = (v0 + u[:, None] * (v1 - v0)) + v[:, None] * (v2 - v0)
        w = area[f] / (kk * kk).astype(F32)
    return {'points': pts.astype(F32), 'face': f.astype(np.int32), 'bary': np.stack([b0, u, v], 1).astype(F32), 'weight': w.astype(F32),
            'total': int(n.sum()), 'flags': flags}


def used_vertices(verts, faces):
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ok, _ = participating(verts, faces)
    used = np.zeros(len(verts), bool)
    used[faces[ok].ravel()] = True
    return verts[used]


def one_way(va, fa, vb, fb, spacing, include_vertices=True):
    """mesh.distance's figures for one direction, plus the d2 and weights they are made of"""
    s = sample(va, fa, spacing)
    pts, w = s['points'], s['weight']
    if include_vertices:
        extra = used_vertices(va, fa)
        pts, w = np.concatenate([pts, extra]), np.concatenate([w, np.zeros(len(extra), F32)])
    r = closest(vb, fb, pts)
    d2, w = r['dist2'].astype(np.float64), w.astype(np.float64)
    i = int(np.nonzero(r['dist2'] == r['dist2'].max())[0][0])
    area = w.sum()
    return {'max': math.sqrt(d2[i]), 'mean': float((w * np.sqrt(d2)).sum() / area), 'rms': math.sqrt((w * d2).sum() / area),
            'n_samples': s['total'], 'max_point': tuple(float(x) for x in pts[i]), 'max_face': int(r['face'][i])}


def distance(va, fa, vb, fb, spacing, symmetric=True, include_vertices=True):
    out = {'a_to_b': one_way(va, fa, vb, fb, spacing, include_vertices)}
    if symmetric:
        out['b_to_a'] = one_way(vb, fb, va, fa, spacing, include_vertices)
    out['hausdorff'] = max(d['max'] for k, d in out.items())
    return out
