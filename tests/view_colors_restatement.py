"""NumPy restatement of the multi-view colour fusion (cnerf_view_colors_*; rules in include/customnerf_hip.h), written from the rules: float32
with one rounding per written operation in the written order, the views summed in index order, so that the state, the counts and the
resolved colours are bit-equal to the device's.  One view at a time, vectorised over the points.  Also the two scenes that the host and
the GPU tests share: random views of an analytic coloured sphere laced with the rule's edge cases, and that sphere as a mesh seen from
the 14 cameras of the TSDF tests."""
import functools

import numpy as np

from tsdf_restatement import CONVENTIONS, DEPTH_KINDS, look_at, sphere_cameras  # noqa: F401

f32 = np.float32
TAPS = [(0, 0), (1, 0), (0, 1), (1, 1)]                                          # (i, j) of c00, c10, c01, c11: pixel (x0 + i, y0 + j)


def bilerp(a00, a10, a01, a11, ax, ay, gx, gy):
    """(a00 gx + a10 ax) gy + (a01 gx + a11 ax) ay, every operation rounded to float32"""
    return ((a00 * gx + a10 * ax) * gy + (a01 * gx + a11 * ax) * ay).astype(f32)


def footprint(points, c2w, intrinsics, H, W, convention='nerfstudio', near=0.01):
    """steps 1-2 of the rule and the lengths of step 3 for one view: dict of d (three float32 [M]), z, ln = |d|, ax, ay, ix, iy (int64, 0
    where not ok) and ok: the point lies in front of the camera and its 2 x 2 footprint in the image"""
    m = np.asarray(c2w, f32)[:3, :4]
    fx, fy, cx, cy = (f32(x) for x in intrinsics)
    near, half = f32(near), f32(0.5)
    p = [np.ascontiguousarray(points[:, a], f32) for a in range(3)]
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
        u, v = X - half, Y - half
        xf, yf = np.floor(u), np.floor(v)
        ax, ay = (u - xf).astype(f32), (v - yf).astype(f32)
        ok = (z >= near) & (xf >= 0) & (xf <= f32(W - 2)) & (yf >= 0) & (yf <= f32(H - 2))
        ix = np.where(ok, xf, 0).astype(np.int64)
        iy = np.where(ok, yf, 0).astype(np.int64)
        ok &= (ix + 1 < W) & (iy + 1 < H)
        ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return dict(d=d, z=z, ln=ln, ax=ax, ay=ay, ix=np.where(ok, ix, 0), iy=np.where(ok, iy, 0), ok=ok)


def accumulate(state, seen, points, normals, images, depth, c2w, intrinsics, depth_tol, convention='nerfstudio', depth_kind='z',
               weights=None, power=2, min_cos=0.2, near=0.01):
    """state float32 [M, 4] (sum w r, sum w g, sum w b, sum w) and seen uint32 [M], updated in place by the views images [N, H, W, 3] /
    depth [N, H, W] / c2w [N, 3|4, 4] in index order -> (state, seen)"""
    images, depth = np.asarray(images, f32), np.asarray(depth, f32)
    c2w = np.asarray(c2w, f32)
    N, H, W = depth.shape
    weights = None if weights is None else np.asarray(weights, f32).reshape(depth.shape)
    tol, min_cos = f32(depth_tol), f32(min_cos)
    n = [np.ascontiguousarray(normals[:, a], f32) for a in range(3)]
    for v in range(N):
        fp = footprint(points, c2w[v], intrinsics, H, W, convention, near)
        d, ax, ay, ix, iy, ok = fp['d'], fp['ax'], fp['ay'], fp['ix'], fp['iy'], fp['ok'].copy()
        with np.errstate(all="ignore"):
            r = fp['z'] if DEPTH_KINDS[depth_kind] == 0 else fp['ln']
            for i, j in TAPS:
                D = depth[v][iy + j, ix + i]
                ok &= (D > 0) & (D < np.inf) & (np.abs(D - r) <= tol)
            cos = (-((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]) / fp['ln']).astype(f32)
            ok &= cos > min_cos
            w = cos.copy()
            for _ in range(1, int(power)):
                w = (w * cos).astype(f32)
            gx, gy = (f32(1.0) - ax).astype(f32), (f32(1.0) - ay).astype(f32)
            if weights is not None:
                w = (w * bilerp(*[weights[v][iy + j, ix + i] for i, j in TAPS], ax, ay, gx, gy)).astype(f32)
            ok &= (w > 0) & (w < np.inf)
            for k in range(3):
                ck = bilerp(*[images[v][iy + j, ix + i, k] for i, j in TAPS], ax, ay, gx, gy)
                wc = (w * ck).astype(f32)
                state[ok, k] = (state[ok, k] + wc[ok]).astype(f32)
            state[ok, 3] = (state[ok, 3] + w[ok]).astype(f32)
            seen[ok] += np.uint32(1)
    return state, seen


def resolve(state, seen, fallback=None, fill=(0.0, 0.0, 0.0)):
    """-> (out float32 [M, 3], counts int64 [3]: the points seen by 0, 1 and >= 2 views)"""
    have = state[:, 3] > 0
    other = np.asarray(fallback, f32) if fallback is not None else np.broadcast_to(np.asarray(fill, f32), (len(state), 3))
    with np.errstate(all="ignore"):
        out = np.where(have[:, None], state[:, :3] / np.where(have, state[:, 3], f32(1))[:, None], other).astype(f32)
    cls = np.minimum(seen, 2)
    return out, np.array([(cls == k).sum() for k in range(3)], np.int64)


def fuse(points, normals, images, depth, c2w, intrinsics, depth_tol, **kw):
    """zeroed state and counts -> (state, seen) of all the views"""
    return accumulate(np.zeros((len(points), 4), f32), np.zeros(len(points), np.uint32), points, normals, images, depth, c2w, intrinsics,
                      depth_tol, **kw)


# ------------------------------------------------------------------------------------------------ the coloured sphere, ray-traced
RADIUS = 0.3


def sphere_color(x):
    """the analytic colour 0.5 + 0.5 x / |x| of the sphere's surface point in direction x (float64)"""
    x = np.asarray(x, np.float64)
    return 0.5 + 0.5 * x / np.linalg.norm(x, axis=-1, keepdims=True)


def sphere_render(c2w, H, W, intrinsics, radius=RADIUS):
    """The sphere round the origin, coloured by sphere_color, ray-traced in float64 through the pixel centres of a nerfstudio camera ->
    (image [H, W, 3] float32, black where the ray misses; distance along the ray [H, W] float32, +inf where it misses; camera-axis depth
    likewise)"""
    fx, fy, cx, cy = intrinsics
    m = np.asarray(c2w, np.float64)
    iy, ix = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    cam = np.stack([(ix - cx) / fx, -(iy - cy) / fy, -np.ones_like(ix)], -1)      # z = 1 along the axis
    scale = np.linalg.norm(cam, axis=-1)
    d = (cam / scale[..., None]) @ m[:3, :3].T
    o = m[:3, 3]
    b = d @ o
    disc = b * b - (o @ o - radius * radius)
    with np.errstate(all="ignore"):
        t = -b - np.sqrt(disc)
        hit = (disc > 0) & (t > 0)
        x = o + np.where(hit, t, 1.0)[..., None] * d
        img = np.where(hit[..., None], sphere_color(x), 0.0)
    t = np.where(hit, t, np.inf)
    return img.astype(f32), t.astype(f32), (t / scale).astype(f32)


def to_ngp(c2w):
    """the same camera in the 'ngp' convention (+z forward, y down): columns y and z change sign"""
    m = np.array(c2w, f32)
    m[..., :3, 1:3] *= -1
    return m


# ------------------------------------------------------------------------------------------------ scene 1: random views, laced with the edge cases
H, W = 40, 48                                                                    # H != W
K = (60.0, 55.0, 24.3, 19.6)
NPTS, NEAR, TOL, MIN_COS = 1000, 0.25, 2.0 ** -5, 0.2
# What view 0 alone does with each laced point: 1 it adds to the point, 0 it does not.  'weight0' is seen only without pixel weights.
EDGE_CASES = {'control': 1, 'behind': 0, 'under_near': 0, 'over_near': 1, 'border_out': 0, 'border_in': 1, 'mixed_bad': 0, 'nan': 0,
              'zero': 0, 'inf': 0, 'negative': 0, 'occluded': 0, 'exact_tol': 1, 'past_tol': 0, 'cos_below': 0, 'cos_above': 1, 'weight0': 0}


@functools.lru_cache(maxsize=None)
def edge_scene(n_views, convention, depth_kind):
    """dict(points, normals [NPTS, 3], images [N, H, W, 3], depth [N, H, W], weights [N, H, W], cams [N, 3, 4], edge {name: index}).
    Cameras round the sphere looking at it; depths are the sphere's, analytic, seeded with +inf, NaN, 0, negative and displaced pixels;
    weights with zeros.  Most points lie on the sphere with jittered radial normals.  View 0 looks down -z from (0, 0, 1.5); the edge
    points are placed in front of it (1.2 along its axis unless the case says otherwise), each on pixels of its own, and the depth and
    weight of view 0 on their footprints are painted so that the case's condition alone decides (EDGE_CASES)."""
    rng = np.random.default_rng(300 + n_views)
    eyes = rng.standard_normal((n_views, 3))
    eyes = eyes / np.linalg.norm(eyes, axis=1, keepdims=True) * rng.uniform(1.0, 1.6, (n_views, 1))
    eyes[0] = (0.0, 0.0, 1.5)
    studio = np.stack([look_at(e) for e in eyes])
    rendered = [sphere_render(c, H, W, K) for c in studio]
    images = np.stack([r[0] for r in rendered])
    images[images.sum(-1) == 0] = (0.9, 0.1, 0.8)                                # a background that would show if it bled in
    depth = np.stack([r[1] if depth_kind == 'ray' else r[2] for r in rendered])
    kind = rng.random(depth.shape)
    depth[kind < 0.03] = np.inf
    depth[(kind >= 0.03) & (kind < 0.05)] = np.nan
    depth[(kind >= 0.05) & (kind < 0.06)] = 0.0
    depth[(kind >= 0.06) & (kind < 0.07)] = -0.7
    shift = (kind >= 0.07) & (kind < 0.12)
    depth[shift] += rng.uniform(-2 * TOL, 2 * TOL, depth.shape).astype(f32)[shift]
    weights = rng.uniform(0.25, 2.0, depth.shape).astype(f32)
    weights[rng.random(depth.shape) < 0.1] = 0.0
    cams = studio if convention == 'nerfstudio' else to_ngp(studio)

    dirs = rng.standard_normal((NPTS, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    points = (RADIUS * dirs).astype(f32)
    normals = dirs + 0.2 * rng.standard_normal((NPTS, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(f32)

    m0 = studio[0].astype(np.float64)

    def at_pixel(X, Y, z):                                                       # the world point that view 0 sees at (X, Y), z along its axis
        return m0[:, :3] @ np.array([(X - K[2]) / K[0] * z, -(Y - K[3]) / K[1] * z, -z]) + m0[:, 3]

    # name -> (X, Y, z); every footprint has pixels of its own
    where = {'control': (4.3, 4.6, 1.2), 'behind': (10.3, 4.6, -1.0), 'under_near': (16.3, 4.6, NEAR - 1e-4), 'over_near': (22.3, 4.6, NEAR + 1e-4),
             'border_out': (0.25, 12.6, 1.2), 'border_in': (0.75, 20.6, 1.2), 'mixed_bad': (10.3, 12.6, 1.2), 'nan': (16.3, 12.6, 1.2),
             'zero': (22.3, 12.6, 1.2), 'inf': (28.3, 12.6, 1.2), 'negative': (34.3, 12.6, 1.2), 'occluded': (40.3, 12.6, 1.2),
             'exact_tol': (4.3, 28.6, 1.2), 'past_tol': (10.3, 28.6, 1.2), 'cos_below': (16.3, 28.6, 1.2), 'cos_above': (22.3, 28.6, 1.2),
             'weight0': (28.3, 28.6, 1.2)}
    assert set(where) == set(EDGE_CASES)
    edge = {name: 7 + 57 * k for k, name in enumerate(where)}                    # spread over the waves, none at a wave's start
    for name, (X, Y, z) in where.items():
        p = at_pixel(X, Y, z)
        e = m0[:, 3] - p
        e /= np.linalg.norm(e)                                                   # towards the camera
        if name in ('cos_below', 'cos_above'):
            side = np.cross(e, [0.0, 1.0, 0.0])
            side /= np.linalg.norm(side)
            c = MIN_COS + (1e-4 if name == 'cos_above' else -1e-4)
            e = c * e + np.sqrt(1.0 - c * c) * side
        if name == 'behind':
            e = -e                                                               # would face the camera if the camera could look back
        points[edge[name]], normals[edge[name]] = p, e
    idx = np.array(list(edge.values()))
    fp = footprint(points[idx], cams[0], K, H, W, convention, NEAR)
    r = fp['z'] if depth_kind == 'z' else fp['ln']
    nan, inf, tol = f32(np.nan), f32(np.inf), f32(TOL)

    def painted(name, r):                                                        # the four footprint depths of view 0, in TAPS order
        D = [r, r, r, r]
        if name == 'mixed_bad':
            D[1:] = [nan, f32(0.0), inf]
        elif name in ('nan', 'zero', 'inf', 'negative'):
            D[('negative', 'nan', 'zero', 'inf').index(name)] = {'nan': nan, 'zero': f32(0.0), 'inf': inf, 'negative': f32(-0.5)}[name]
        elif name == 'occluded':
            D = [r - f32(2.0) * tol] * 4                                         # a surface in front of the point
        elif name == 'exact_tol':
            D = [r + tol, r - tol, r + tol, r]                                   # exact sums: 1 <= r < 1.9 and tol is a power of two
        elif name == 'past_tol':
            D[3] = np.nextafter(r + tol, inf)                                    # one ulp past the tolerance
        return D
    for q, name in enumerate(where):
        if name in ('behind', 'under_near', 'border_out'):
            assert not fp['ok'][q], name
            continue
        assert fp['ok'][q] and (name == 'over_near' or 1.0 <= r[q] < 1.9), name
        for D, (i, j) in zip(painted(name, r[q]), TAPS):
            depth[0, fp['iy'][q] + j, fp['ix'][q] + i] = D
            weights[0, fp['iy'][q] + j, fp['ix'][q] + i] = 0.0 if name == 'weight0' else 1.0
    return dict(points=points, normals=normals, images=images, depth=depth, weights=weights, cams=cams, edge=edge)


# ------------------------------------------------------------------------------------------------ scene 2: the sphere as a mesh, 14 cameras
IMG, FOCAL = 64, 110.0
INTRINSICS = (FOCAL, FOCAL, IMG / 2.0, IMG / 2.0)
SPHERE_TOL = 0.05           # a vertex is a convex tip of the inscribed polyhedron: the faces round it lie up to 0.02 deeper a pixel away
SPHERE_LEVEL = 3                                                                 # 258 vertices, 512 faces


def sphere_mesh():
    """(verts [V, 3] float32 on the sphere of RADIUS, faces [F, 3] int32, unit normals [V, 3] float32) of the subdivided octahedron"""
    from mesh_testlib import octahedron_sphere
    unit, faces = octahedron_sphere(SPHERE_LEVEL)
    return (unit * RADIUS).astype(f32), faces, unit.astype(f32)


def sphere_images():
    """[14, IMG, IMG, 3] float32: the ray-traced coloured sphere from sphere_cameras()"""
    return np.stack([sphere_render(c, IMG, IMG, INTRINSICS)[0] for c in sphere_cameras()])
