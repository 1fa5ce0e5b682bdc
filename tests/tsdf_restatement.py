"""NumPy restatement of the TSDF fusion (cnerf_tsdf_*; rules in include/customnerf_hip.h), written from the rules: float32 with one rounding
per written operation in the written order, the views summed in index order, so that acc, weight, the finalised volume and the face flags are
bit-equal to the device's.  One view at a time, vectorised over the lattice.  Also the analytic sphere scene that the host and the GPU tests
share."""
import numpy as np

f32 = np.float32
CONVENTIONS = {'nerfstudio': 0, 'ngp': 1}
DEPTH_KINDS = {'z': 0, 'ray': 1}


def points(shape, origin, spacing):
    """p_b = org_b + (float) idx_b sp_b for every lattice point, z fastest: three float32 [n]"""
    idx = np.meshgrid(*[np.arange(n, dtype=np.int64) for n in shape], indexing="ij")
    return [(f32(origin[b]) + idx[b].ravel().astype(f32) * f32(spacing[b])).astype(f32) for b in range(3)]


def integrate(state, shape, origin, spacing, trunc, depth, c2w, intrinsics, convention='nerfstudio', depth_kind='ray', weights=None,
              near=0.01):
    """state float32 [n, 2] (acc, weight), updated in place by the views depth [N, H, W] / c2w [N, 3|4, 4] in index order -> state"""
    depth = np.asarray(depth, f32)
    depth = depth[None] if depth.ndim == 2 else depth
    c2w = np.asarray(c2w, f32)
    c2w = c2w[None] if c2w.ndim == 2 else c2w
    weights = None if weights is None else np.asarray(weights, f32).reshape(depth.shape)
    N, H, W = depth.shape
    fx, fy, cx, cy = (f32(x) for x in intrinsics)
    trunc, near = f32(trunc), f32(near)
    p = points(shape, origin, spacing)
    acc, wsum = state[:, 0], state[:, 1]
    for v in range(N):
        m = c2w[v][:3, :4]
        with np.errstate(all="ignore"):
            d = [p[a] - m[a, 3] for a in range(3)]
            c = [(m[0, k] * d[0] + m[1, k] * d[1]) + m[2, k] * d[2] for k in range(3)]
            if CONVENTIONS[convention] == 0:
                z = -c[2]
                Y = cy + f32(-1.0) * (fy * (c[1] / z))
            else:
                z = c[2]
                Y = cy + fy * (c[1] / z)
            X = cx + fx * (c[0] / z)
            ok = (z >= near) & (X >= 0) & (X < f32(W)) & (Y >= 0) & (Y < f32(H))
            ix = np.where(ok, np.floor(X), 0).astype(np.int64)
            iy = np.where(ok, np.floor(Y), 0).astype(np.int64)
            ok &= (ix < W) & (iy < H)
            ix, iy = np.where(ok, ix, 0), np.where(ok, iy, 0)
            D = depth[v][iy, ix]
            ok &= D > 0                                                          # NaN, 0 and negative pixels say nothing; +inf is free space
            w = weights[v][iy, ix] if weights is not None else np.ones_like(D)
            ok &= (w > 0) & (w < np.inf)
            r = z if DEPTH_KINDS[depth_kind] == 0 else np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            sdf = (D - r).astype(f32)
            ok &= ~(sdf < -trunc)
            s = -np.minimum(f32(1.0), (sdf / trunc).astype(f32))
            ws = (w * s).astype(f32)
            acc[ok] = (acc[ok] + ws[ok]).astype(f32)
            wsum[ok] = (wsum[ok] + w[ok]).astype(f32)
    return state


def finalize(state, shape, fill=-1.0):
    """-> (volume float32 [nx, ny, nz], observed points)"""
    seen = state[:, 1] > 0
    with np.errstate(all="ignore"):
        vol = np.where(seen, state[:, 0] / np.where(seen, state[:, 1], f32(1)), f32(fill)).astype(f32)
    return vol.reshape(shape), int(seen.sum())


def face_keep(state, shape, origin, spacing, verts, faces):
    """bool [F]: the lattice cell that holds the face's centroid has eight observed corners"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    seen = (state[:, 1] > 0).reshape(shape)
    q = []
    with np.errstate(all="ignore"):
        for b in range(3):
            c = (((v[fc[:, 0], b] + v[fc[:, 1], b]) + v[fc[:, 2], b]) / f32(3.0)).astype(f32)
            k = np.floor(((c - f32(origin[b])) / f32(spacing[b])).astype(f32))
            q.append(np.clip(np.where(np.isnan(k), 0, k), 0, shape[b] - 2).astype(np.int64))
    keep = np.ones(len(fc), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                keep &= seen[q[0] + dx, q[1] + dy, q[2] + dz]
    return keep


def compact(verts, faces, keep):
    """the kept faces in their order and the vertices they use in theirs -> (verts, faces int32)"""
    fc = np.asarray(faces, np.int64)[keep]
    used = np.zeros(len(verts), bool)
    used[fc.ravel()] = True
    new = np.cumsum(used) - 1
    return np.asarray(verts)[used], new[fc].astype(np.int32)


# ------------------------------------------------------------------------------------------------ the sphere scene of the tests
RADIUS, RES, IMG, FOCAL = 0.3, 32, 64, 110.0
SHAPE = (RES, RES, RES)
ORIGIN = (-0.5, -0.5, -0.5)
STEP = 1.0 / (RES - 1)
SPACING = (STEP, STEP, STEP)
TRUNC = 4 * STEP
INTRINSICS = (FOCAL, FOCAL, IMG / 2.0, IMG / 2.0)


def look_at(eye):
    """[3, 4] float32 nerfstudio camera-to-world (x right, y up, looks down -z) at `eye`, looking at the origin"""
    eye = np.asarray(eye, np.float64)
    back = eye / np.linalg.norm(eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(back[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    return np.concatenate([np.stack([right, np.cross(back, right), back], 1), eye[:, None]], 1).astype(f32)


def sphere_cameras():
    """the 14 views: six along the axes at distance 2, eight from the corners (+-1.2, +-1.2, +-1.2)"""
    eyes = [(2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2)]
    eyes += [(a, b, c) for a in (1.2, -1.2) for b in (1.2, -1.2) for c in (1.2, -1.2)]
    return np.stack([look_at(e) for e in eyes])


def sphere_depth(c2w, kind, radius=RADIUS, size=IMG, intrinsics=INTRINSICS):
    """analytic depth map [size, size] of the sphere round the origin through the pixel centres, computed in float64 and cast to float32:
    'ray' the distance along the ray, 'z' the camera-axis depth; +inf where the ray misses"""
    fx, fy, cx, cy = intrinsics
    m = np.asarray(c2w, np.float64)
    iy, ix = np.meshgrid(np.arange(size) + 0.5, np.arange(size) + 0.5, indexing="ij")
    cam = np.stack([(ix - cx) / fx, -(iy - cy) / fy, -np.ones_like(ix)], -1)      # z = 1 along the axis
    scale = np.linalg.norm(cam, axis=-1)
    d = (cam / scale[..., None]) @ m[:3, :3].T
    o = m[:3, 3]
    b = d @ o
    disc = b * b - (o @ o - radius * radius)
    with np.errstate(all="ignore"):
        t = -b - np.sqrt(disc)
    t = np.where((disc > 0) & (t > 0), t, np.inf)
    return (t if kind == 'ray' else t / scale).astype(f32)


def fuse_sphere(kind):
    """the scene fused by the restatement -> state [n, 2]"""
    cams = sphere_cameras()
    depth = np.stack([sphere_depth(c, kind) for c in cams])
    state = np.zeros((RES ** 3, 2), f32)
    return integrate(state, SHAPE, ORIGIN, SPACING, TRUNC, depth, cams, INTRINSICS, 'nerfstudio', kind)
