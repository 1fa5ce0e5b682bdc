"""NumPy restatement of the mesh rasteriser (cnerf_mesh_raster_*; rules in include/customnerf_hip.h), written from the rules: projection and
snapping in float32 with one rounding per operation in the written order, coverage and the winner exact in int64, depth and barycentrics in
float32, so that face, depth and bary are bit-equal to the device's.  One face at a time, vectorised over its candidate pixels."""
import numpy as np

f32 = np.float32
CONVENTIONS = {'nerfstudio': 0, 'ngp': 1}
CULL = {'none': 0, 'back': 1, 'front': 2}
LIMIT = 2 ** 28


def project(verts, c2w, intrinsics, convention='nerfstudio', near=0.01):
    """per vertex: (xi, yi int64 [V] (0 where not ok), q float32 [V] = 1 / z, ok bool [V], z float32 [V])"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    m = np.asarray(c2w, f32)[:3, :4]
    fx, fy, cx, cy = (f32(x) for x in intrinsics)
    with np.errstate(all="ignore"):
        d = [v[:, a] - m[a, 3] for a in range(3)]
        c = [(m[0, k] * d[0] + m[1, k] * d[1]) + m[2, k] * d[2] for k in range(3)]
        if CONVENTIONS[convention] == 0:
            z = -c[2]
            Y = cy + f32(-1.0) * (fy * (c[1] / z))
        else:
            z = c[2]
            Y = cy + fy * (c[1] / z)
        X = cx + fx * (c[0] / z)
        rx, ry = np.rint(X * f32(256.0)), np.rint(Y * f32(256.0))
        ok = np.isfinite(z) & (z >= f32(near)) & np.isfinite(X) & np.isfinite(Y) & (np.abs(rx) < LIMIT) & (np.abs(ry) < LIMIT)
        q = (f32(1.0) / z).astype(f32)
    xi = np.where(ok, rx, 0).astype(np.int64)
    yi = np.where(ok, ry, 0).astype(np.int64)
    return xi, yi, q, ok, z.astype(f32)


def _floor_div(a, b):
    return a // b                                                            # Python and NumPy integer division floor


def _face_cover(x, y, q, H, W, cull):
    """One face (x, y int [3], q float32 [3], input order) -> None, or (ix, iy int64 [n], depth float32 [n], beta float32 [n, 3] in input
    order) of the covered pixels, plus whether it is front-facing."""
    x = [int(a) for a in x]
    y = [int(a) for a in y]
    A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if A == 0 or (cull == 1 and A > 0) or (cull == 2 and A < 0):
        return None
    perm = [0, 1, 2]
    if A < 0:
        perm = [0, 2, 1]
        A = -A
    x, y, q = [x[p] for p in perm], [y[p] for p in perm], [q[p] for p in perm]
    x0 = max(-_floor_div(-(min(x) - 128), 256), 0)                           # ceil
    x1 = min(_floor_div(max(x) - 128, 256), W - 1)
    y0 = max(-_floor_div(-(min(y) - 128), 256), 0)
    y1 = min(_floor_div(max(y) - 128, 256), H - 1)
    if x0 > x1 or y0 > y1:
        return None
    iy, ix = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
    px, py = 256 * ix + 128, 256 * iy + 128
    E, inside = [], np.ones(px.shape, bool)
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        dx, dy = x[j] - x[i], y[j] - y[i]
        e = dx * (py - y[i]) - dy * (px - x[i])
        top_left = dy < 0 or (dy == 0 and dx > 0)
        inside &= (e > 0) | ((e == 0) & top_left)
        E.append(e)
    if not inside.any():
        return None
    ix, iy = ix[inside], iy[inside]
    Af = f32(np.int64(A))
    with np.errstate(all="ignore"):
        bq = [((E[k][inside].astype(f32) / Af) * f32(q[k])).astype(f32) for k in range(3)]
        depth = (f32(1.0) / ((bq[0] + bq[1]) + bq[2])).astype(f32)
        beta = np.zeros((len(ix), 3), f32)
        for k in range(3):
            beta[:, perm[k]] = bq[k] * depth
    return ix, iy, depth, beta


def visibility(verts, faces, c2w, intrinsics, H, W, convention='nerfstudio', near=0.01, cull='none', count_cover=False):
    """-> dict(face [H, W] int32 (-1: none), depth [H, W] float32 (+inf: none), bary [H, W, 3] float32 (0: none), dropped int,
    bad bool: a face index outside [0, V), the outputs are then all-empty; with count_cover also cover [H, W] int64: the number of faces
    covering each pixel)"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    xi, yi, q, ok, _ = project(v, c2w, intrinsics, convention, near)
    key = np.full((H, W), np.iinfo(np.uint64).max, np.uint64)
    bary = np.zeros((H, W, 3), f32)
    cover = np.zeros((H, W), np.int64)
    dropped, bad = 0, False
    for f, tri in enumerate(fc):
        if (tri < 0).any() or (tri >= V).any():
            bad = True
            continue
        if not ok[tri].all():
            dropped += 1
            continue
        r = _face_cover(xi[tri], yi[tri], q[tri], H, W, CULL[cull])
        if r is None:
            continue
        ix, iy, depth, beta = r
        k = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        win = k < key[iy, ix]
        key[iy[win], ix[win]] = k[win]
        bary[iy[win], ix[win]] = beta[win]
        cover[iy, ix] += 1
    hit = key != np.iinfo(np.uint64).max
    face = np.where(hit, (key & np.uint64(0xffffffff)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (key >> np.uint64(32)).astype(np.uint32).view(f32), f32(np.inf)).astype(f32)
    bary[~hit] = 0
    if bad:
        face[:], depth[:], bary[:] = -1, np.inf, 0
    out = dict(face=face, depth=depth, bary=bary, dropped=dropped, bad=bad)
    if count_cover:
        out['cover'] = cover
    return out


def to_u8(x):
    """round(clamp(x, 0, 1) 255), half to even, NaN -> 0"""
    with np.errstate(all="ignore"):
        x = np.asarray(x, f32)
        c = np.minimum(np.maximum(np.where(np.isnan(x), f32(0), x), f32(0)), f32(1))
        return np.rint(c * f32(255.0)).astype(np.uint8)


def _mix(b, a0, a1, a2):
    """(b0 a0 + b1 a1) + b2 a2 per component, float32; b [n, 3], a_k [n, C]"""
    return ((b[:, 0:1] * a0 + b[:, 1:2] * a1) + b[:, 2:3] * a2).astype(f32)


def _unit(x):
    with np.errstate(all="ignore"):
        l2 = ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]).astype(f32)
        ok = (l2 > 0) & np.isfinite(l2)
        l = np.sqrt(np.where(ok, l2, f32(1))).astype(f32)
        return (x / l[:, None]).astype(f32), ok


def shade(vis, verts, faces, mode, colors=None, uvs=None, texture=None, normals=None, depth_range=(0.0, 1.0), bg=(0, 0, 0)):
    """-> (image [H, W, 3] uint8, mask [H, W] uint8 255 / 0) from the visibility dict; mode 'colors', 'texture', 'normals' or 'depth'"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    face, depth, bary = vis['face'], vis['depth'], vis['bary']
    H, W = face.shape
    image = np.empty((H, W, 3), np.uint8)
    image[:] = np.asarray(bg, np.uint8)
    hit = face >= 0
    mask = np.where(hit, 255, 0).astype(np.uint8)
    if not hit.any():
        return image, mask
    f = face[hit].astype(np.int64)
    b = bary[hit].astype(f32)
    tri = fc[f]
    with np.errstate(all="ignore"):
        if mode == 'colors':
            c = np.asarray(colors, np.uint8).astype(f32)
            x = _mix(b, c[tri[:, 0]], c[tri[:, 1]], c[tri[:, 2]]) / f32(255.0)
        elif mode == 'texture':
            uv = np.asarray(uvs, f32).reshape(-1, 3, 2)[f]
            t = np.asarray(texture, np.uint8).astype(f32)
            R = t.shape[0]
            u = _mix(b, uv[:, 0], uv[:, 1], uv[:, 2])
            px = (u[:, 0] * f32(R) - f32(0.5)).astype(f32)
            py = ((f32(1.0) - u[:, 1]) * f32(R) - f32(0.5)).astype(f32)
            fx0, fy0 = np.floor(px), np.floor(py)
            wx, wy = (px - fx0).astype(f32)[:, None], (py - fy0).astype(f32)[:, None]
            X = np.clip(np.where(np.isnan(fx0), -32768, fx0), -32768, 32768).astype(np.int64)
            Y = np.clip(np.where(np.isnan(fy0), -32768, fy0), -32768, 32768).astype(np.int64)

            def at(xx, yy):
                return t[np.clip(yy, 0, R - 1), np.clip(xx, 0, R - 1)]
            one = f32(1.0)
            x = ((((one - wx) * (one - wy)) * at(X, Y) + (wx * (one - wy)) * at(X + 1, Y)) + ((one - wx) * wy) * at(X, Y + 1)) \
                + (wx * wy) * at(X + 1, Y + 1)
            x = x.astype(f32) / f32(255.0)
        elif mode == 'normals':
            nv = np.asarray(normals, f32).reshape(-1, 3)
            n, ok = _unit(_mix(b, nv[tri[:, 0]], nv[tri[:, 1]], nv[tri[:, 2]]))
            e1, e2 = v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]]
            g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(f32)
            gn, okg = _unit(g)
            n = np.where(ok[:, None], n, np.where(okg[:, None], gn, f32(0)))
            x = f32(0.5) + f32(0.5) * n
        else:
            d0, d1 = f32(depth_range[0]), f32(depth_range[1])
            x = np.repeat(((depth[hit] - d0) / (d1 - d0))[:, None], 3, 1)
        image[hit] = to_u8(x)
    return image, mask
