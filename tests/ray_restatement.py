"""NumPy restatement of the ray rules of csrc/mesh_bvh.hip (include/customnerf_hip.h, cnerf_mesh_bvh_raycast / _occluded) and of
mesh.ao_directions / mesh.ao_rays / mesh.ambient_occlusion: the watertight ray/triangle rule in float32 with one rounding per written operation and
its float64 fallback, brute force over every face that takes part (the smallest t, the smallest face index on a tie; the any-hit bit).  No
tree here: the definition of the result does not mention one."""
import math

import numpy as np

from bvh_restatement import participating

F32 = np.float32
CULL = {'none': 0, 'back': 1, 'front': 2}


def ray_setup(origins, dirs):
    """-> (ok [Q], kx, ky, kz [Q] int, Sx, Sy, Sz [Q] float32) of the rays; ok = not degenerate by o and d alone"""
    o, d = np.asarray(origins, F32).reshape(-1, 3), np.asarray(dirs, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        kz = np.argmax(np.abs(np.where(np.isnan(d), F32(0), d)), 1)            # the first largest: the lowest axis on a tie
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        q = np.arange(len(d))
        dz = d[q, kz]
        swap = dz < 0
        kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
        Sx, Sy, Sz = d[q, kx] / dz, d[q, ky] / dz, F32(1) / dz
        ok = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.abs(dz) > 0) & np.isfinite(Sx) & np.isfinite(Sy) & np.isfinite(Sz)
    return ok, kx, ky, kz, Sx.astype(F32), Sy.astype(F32), Sz.astype(F32)


def ray_faces(a, b, c, origins, dirs):
    """the rule of every ray [Q] against every face [F] (a, b, c: [F, 3]) -> dict of [Q, F] arrays: t, det, U, V, W (float32), inside (no
    mixed strict signs) and fallback (the float64 branch was taken).  Degenerate rays are not treated here."""
    o = np.asarray(origins, F32).reshape(-1, 1, 3)
    _, kx, ky, kz, Sx, Sy, Sz = ray_setup(origins, dirs)
    Sx, Sy, Sz = Sx[:, None], Sy[:, None], Sz[:, None]
    with np.errstate(all="ignore"):
        def shear(p):
            P = np.asarray(p, F32)[None] - o                                    # [Q, F, 3]
            pz = np.take_along_axis(P, kz[:, None, None], 2)[..., 0]
            px = np.take_along_axis(P, kx[:, None, None], 2)[..., 0] - Sx * pz
            py = np.take_along_axis(P, ky[:, None, None], 2)[..., 0] - Sy * pz
            return px, py, pz
        (Ax, Ay, Akz), (Bx, By, Bkz), (Cx, Cy, Ckz) = shear(a), shear(b), shear(c)
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        neg, pos = (U < 0) | (V < 0) | (W < 0), (U > 0) | (V > 0) | (W > 0)
        fb = (U == 0) | (V == 0) | (W == 0)
        if fb.any():
            ax, ay, bx, by, cx, cy = (x[fb].astype(np.float64) for x in (Ax, Ay, Bx, By, Cx, Cy))
            Ud, Vd, Wd = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
            neg[fb], pos[fb] = (Ud < 0) | (Vd < 0) | (Wd < 0), (Ud > 0) | (Vd > 0) | (Wd > 0)
            U[fb], V[fb], W[fb] = Ud.astype(F32), Vd.astype(F32), Wd.astype(F32)
        det = (U + V) + W
        Az, Bz, Cz = Sz * Akz, Sz * Bkz, Sz * Ckz
        t = ((U * Az + V * Bz) + W * Cz) / det
    return {'t': t, 'det': det, 'U': U, 'V': V, 'W': W, 'inside': ~(neg & pos), 'fallback': fb}


def _per_ray(x, Q):
    return np.broadcast_to(np.asarray(x, F32), (Q,)).astype(F32)


def cast(verts, faces, origins, dirs, t_min=0.0, t_max=np.inf, culls=('none',), block=256):
    """brute force -> {cull: dict t [Q] float32 (+inf: a miss), face [Q] int32 (-1), bary [Q, 3] float32 (0), occluded [Q] bool}, and under
    'fallbacks' the number of (ray, face) pairs that took the float64 branch"""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    o, d = np.asarray(origins, F32).reshape(-1, 3), np.asarray(dirs, F32).reshape(-1, 3)
    Q = len(o)
    tmin, tmax = _per_ray(t_min, Q), _per_ray(t_max, Q)
    idx = np.nonzero(participating(verts, faces)[0])[0]
    a, b, c = (verts[faces[idx, k]] for k in range(3))
    with np.errstate(all="ignore"):
        live = ray_setup(o, d)[0] & ~(tmin > tmax)
    out = {k: {'t': np.full(Q, np.inf, F32), 'face': np.full(Q, -1, np.int32), 'bary': np.zeros((Q, 3), F32), 'occluded': np.zeros(Q, bool)}
           for k in culls}
    out['fallbacks'] = 0
    if not len(idx):
        return out
    for s in range(0, Q, block):
        e = min(s + block, Q)
        r = ray_faces(a, b, c, o[s:e], d[s:e])
        out['fallbacks'] += int(r['fallback'][live[s:e]].sum())
        with np.errstate(all="ignore"):
            t, det = r['t'], r['det']
            base = r['inside'] & (det != 0) & (tmin[s:e, None] <= t) & (t <= tmax[s:e, None]) & live[s:e, None]
            for k in culls:
                hit = base & {0: True, 1: ~(det < 0), 2: ~(det > 0)}[CULL[k]]
                anyhit = hit.any(1)
                best = np.where(hit, t, np.inf).min(1)
                j = np.argmax(hit & (t == best[:, None]), 1)                    # idx is increasing: the smallest face index
                rows = np.nonzero(anyhit)[0]
                jj = j[rows]
                o_k = out[k]
                o_k['occluded'][s + rows] = True
                o_k['t'][s + rows] = t[rows, jj]
                o_k['face'][s + rows] = idx[jj]
                dj = det[rows, jj]
                o_k['bary'][s + rows] = np.stack([r['U'][rows, jj] / dj, r['V'][rows, jj] / dj, r['W'][rows, jj] / dj], 1)
    return out


def ao_directions(K):
    """mesh.ao_directions: i = 0 .. K - 1, u = (i + 0.5) / K, z = sqrt(1 - u), r = sqrt(u), phi = 2 pi frac(i (sqrt(5) - 1) / 2),
    (r cos phi, r sin phi, z) in float64, rounded once to float32"""
    i = np.arange(int(K), dtype=np.float64)
    u = (i + 0.5) / float(K)
    phi = 2.0 * math.pi * np.mod(i * ((math.sqrt(5.0) - 1.0) / 2.0), 1.0)
    r = np.sqrt(u)
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u)], 1).astype(F32)


def basis(n):
    """the branch-free orthonormal basis of Duff et al. (JCGT 6(1), 2017) about unit normals n [V, 3], float32: (b1, b2)"""
    n = np.asarray(n, F32)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        s = np.copysign(F32(1), nz)
        a = F32(-1) / (s + nz)
        b = (nx * ny) * a
        b1 = np.stack([F32(1) + (s * (nx * nx)) * a, s * b, (-s) * nx], 1)
        b2 = np.stack([b, s + (ny * ny) * a, -ny], 1)
    return b1.astype(F32), b2.astype(F32)


def ao_rays(verts, normals, K, bias):
    """mesh.ao_rays: origins x + bias n and directions (dx b1 + dy b2) + dz n of the K directions of every vertex -> ([V, K, 3], [V, K, 3]);
    n = normals / |normals|"""
    v, n = np.asarray(verts, F32), np.asarray(normals, F32)
    with np.errstate(all="ignore"):
        n = n / np.sqrt((n[:, 0:1] * n[:, 0:1] + n[:, 1:2] * n[:, 1:2]) + n[:, 2:3] * n[:, 2:3])
        b1, b2 = basis(n)
        d = ao_directions(K)
        dirs = (d[None, :, 0:1] * b1[:, None] + d[None, :, 1:2] * b2[:, None]) + d[None, :, 2:3] * n[:, None]
        org = v + F32(bias) * n
    return np.broadcast_to(org[:, None], dirs.shape).astype(F32), dirs.astype(F32)


def used_vertices(verts, faces):
    """mask [V] of the vertices some face that takes part uses"""
    verts, faces = np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    used = np.zeros(len(verts), bool)
    used[faces[participating(verts, faces)[0]].ravel()] = True
    return used


def ambient_occlusion(verts, faces, origins, dirs, radius=np.inf):
    """brute-force AO from rays [V, K, 3] (as ao_rays or the device made them): the share of each vertex's K rays no face stops within
    [0, radius]; 1 for a vertex no valid face uses -> ([V] float32, the escaped counts [V])"""
    V, K = origins.shape[:2]
    occ = cast(verts, faces, origins.reshape(-1, 3), dirs.reshape(-1, 3), 0.0, radius)['none']['occluded'].reshape(V, K)
    free = K - occ.sum(1)
    free[~used_vertices(verts, faces)] = K
    return (free.astype(F32) / F32(K)).astype(F32), free
