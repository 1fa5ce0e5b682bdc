"""NumPy restatement of the projection rule of csrc/mesh_bvh.hip (include/customnerf_hip.h, cnerf_mesh_bvh_project): a composition of the
restated ray rule (ray_restatement.cast: forward along n with cull 'front', backward along -n with cull 'back'), the restated closest-point
rule (bvh_restatement.closest) for the queries both rays miss, and the float32 interpolation and normalisation of the outputs
(atlas_restatement._look is the normalisation, with the sign the atlas gives its view direction).  Brute force over the faces: no tree, and
the second ray is not narrowed — the definition of the result mentions neither."""
import numpy as np

import bvh_restatement as BR
import ray_restatement as RR
from atlas_restatement import _look

F32 = np.float32


def unit(v):
    """(v / sqrt((v0 v0 + v1 v1) + v2 v2), ok) in float32; ok where that sum is positive and finite"""
    d, ok = _look(np.asarray(v, F32).reshape(-1, 3))
    return (-d).astype(F32), ok


def project(verts, faces, normals, x, n, reach):
    """-> dict kind [Q] uint8, face [Q] int32, offset [Q], point [Q, 3], normal [Q, 3] (float32) of the queries (x, n) with `reach` (a number
    or [Q]) against the source mesh (verts, faces) with vertex normals `normals` or None"""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    x, n = np.asarray(x, F32).reshape(-1, 3), np.asarray(n, F32).reshape(-1, 3)
    Q = len(x)
    reach = np.broadcast_to(np.asarray(reach, F32), (Q,)).astype(F32)
    kind, face = np.zeros(Q, np.uint8), np.full(Q, -1, np.int32)
    offset, point, bary = np.zeros(Q, F32), x.copy(), np.zeros((Q, 3), F32)
    with np.errstate(all="ignore"):
        live = np.isfinite(x).all(1) & np.isfinite(n).all(1) & (n != 0).any(1) & (reach >= 0)
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        rows = np.nonzero(live)[0]
        fwd = RR.cast(verts, faces, x[rows], n[rows], 0.0, reach[rows], culls=('front',))['front']
        bwd = RR.cast(verts, faces, x[rows], -n[rows], 0.0, reach[rows], culls=('back',))['back']
        hf, hb = fwd['face'] >= 0, bwd['face'] >= 0
        back = hb & (~hf | (bwd['t'] < fwd['t']))
        front = hf & ~back
        for sel, r, k, sign in ((front, fwd, 1, F32(1)), (back, bwd, 2, F32(-1))):
            q = rows[sel]
            kind[q], face[q], offset[q], bary[q] = k, r['face'][sel], sign * r['t'][sel], r['bary'][sel]
            a, b, c = (verts[faces[r['face'][sel], j]] for j in range(3))
            w = r['bary'][sel]
            point[q] = (w[:, 0:1] * a + w[:, 1:2] * b) + w[:, 2:3] * c
        q = rows[~hf & ~hb]
        cl = BR.closest(verts, faces, x[q])
        ok = (cl['face'] >= 0) & (cl['dist2'] <= (reach[q] * reach[q]) * nn[q])
        q, cf, cp = q[ok], cl['face'][ok], cl['point'][ok]
        r = cp - x[q]
        kind[q], face[q], bary[q], point[q] = 3, cf, cl['bary'][ok], cp
        offset[q] = ((r[:, 0] * n[q, 0] + r[:, 1] * n[q, 1]) + r[:, 2] * n[q, 2]) / nn[q]
        # the normal: interpolated source normals, else the face's, else the query's, else +z
        normal, done = np.tile(np.array([0, 0, 1], F32), (Q, 1)), np.zeros(Q, bool)
        hit = np.nonzero(kind > 0)[0]
        tri = faces[face[hit]]
        a, b, c = (verts[tri[:, j]] for j in range(3))
        if normals is not None:
            nv = np.asarray(normals, F32).reshape(-1, 3)
            w = bary[hit]
            m = (w[:, 0:1] * nv[tri[:, 0]] + w[:, 1:2] * nv[tri[:, 1]]) + w[:, 2:3] * nv[tri[:, 2]]
            u, ok = unit(m)
            normal[hit[ok]], done[hit[ok]] = u[ok], True
        e1, e2 = b - a, c - a
        gn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(F32)
        u, ok = unit(gn)
        take = ok & ~done[hit]
        normal[hit[take]], done[hit[take]] = u[take], True
        u, ok = unit(n)
        take = ok & ~done
        normal[take] = u[take]
    return {'kind': kind, 'face': face, 'offset': offset.astype(F32), 'point': point.astype(F32), 'normal': normal.astype(F32)}


def kinds(kind):
    """the four counts of a kind array"""
    return np.bincount(np.asarray(kind, np.int64).ravel(), minlength=4)[:4]


def store_u8(v):
    """the rounding of the atlas's store kernels (at_u8 of csrc/mesh_texture.hip): rint(min(max(v, 0), 1) * 255) in float32, ties to even"""
    v = np.asarray(v, F32)
    return np.rint(np.minimum(np.maximum(np.where(np.isnan(v), F32(0), v), F32(0)), F32(1)) * F32(255)).astype(np.uint8)


def normal_texels(normal):
    """the RGB8 of an object-space normal map's texels: store_u8(normal * 0.5 + 0.5), the product and the sum rounded to float32"""
    return store_u8(np.asarray(normal, F32) * F32(0.5) + F32(0.5))
