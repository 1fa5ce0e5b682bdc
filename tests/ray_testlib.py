"""What the ray tests share (tests/test_mesh_ray_host.py, tests/test_gpu_mesh_ray.py): small meshes, the watertightness targets of a mesh, and
the mixed ray batch with its brute-force answer (tests/ray_restatement.py), computed once per mesh.  A plain module, NumPy only."""
import functools

import numpy as np

import mc_restatement as R
import ray_restatement as RR
from bvh_restatement import participating
from mesh_testlib import lattice

F32 = np.float32


def mc_sphere(n=21, r=0.9):
    """marching-cubes sphere, wound outwards: n = 21 gives about 3 k faces"""
    (X, Y, Z), sp = lattice((n, n, n), -1.0, 1.0)
    return R.marching_cubes((r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))[:2]


def mc_torus(shape=(30, 28, 20)):
    (X, Y, Z), sp = lattice(shape, -1.0, 1.0)
    q = np.sqrt(X ** 2 + Y ** 2) - 0.6
    return R.marching_cubes((0.25 - np.sqrt(q ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))[:2]


def icosphere(level=2):
    """subdivided icosahedron on the unit sphere, closed, wound outwards, float32"""
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = [np.array(x, float) / np.sqrt(1.0 + p * p) for x in ([-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p],
                                                             [0, 1, -p], [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1])]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2],
         [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                q = v[a] + v[b]
                v.append(q / np.linalg.norm(q))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int32)


def _soup(F, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((3 * F, 3)).astype(np.float32), rng.permutation(3 * F).reshape(F, 3).astype(np.int32)


def _meshes():
    yield ("F0",) + (_soup(2, 1)[0], np.zeros((0, 3), np.int32))                  # an empty tree
    yield ("F1",) + _soup(1, 2)                                                   # one leaf, three NaN records
    yield ("F4",) + _soup(4, 3)                                                   # one full leaf
    yield ("F5",) + _soup(5, 4)                                                   # a second leaf padded with NaN records
    yield ("F13",) + _soup(13, 5)                                                 # four leaves, the last one padded
    sv, sf = mc_sphere(14)
    bad = sf.copy()
    bad[len(sf) // 3, 1] = len(sv)                                                # out of range: left out, the others take part
    bad[len(sf) // 2, 2] = -1
    sv = sv.copy()
    sv[sf[5, 0]] = np.nan                                                         # and every face at a non-finite vertex
    yield "bad_faces", sv, bad
    yield ("sphere",) + mc_sphere()
    yield ("torus",) + mc_torus()


MESHES = list(_meshes())


def mesh(name):
    return next((v, f) for n, v, f in MESHES if n == name)


def finite_box(v, f):
    ok, _ = participating(v, f)
    p = v[f[ok].ravel()] if ok.any() else np.zeros((1, 3), np.float32)
    return p.min(0), p.max(0)


def targets(v, f):
    """every vertex, edge midpoint and face centroid of the faces that take part, rounded to float32"""
    ok, _ = participating(v, f)
    f = f[ok]
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    mids = 0.5 * (v[e[:, 0]].astype(np.float64) + v[e[:, 1]])
    return np.concatenate([v[np.unique(f)], mids, (a + b + c) / 3.0]).astype(np.float32)


def rays_to(origin, tg):
    """rays from one origin through the targets: d = target - origin in float32 (so the target sits at t = 1 up to that rounding)"""
    o = np.broadcast_to(np.asarray(origin, F32), tg.shape).copy()
    return o, (tg - o).astype(F32)


DEGENERATE = [((np.nan, 0, 0), (0, 0, 1), 0.0, np.inf), ((0, np.inf, 0), (0, 0, 1), 0.0, np.inf), ((0, 0, 0), (0, 0, 0), 0.0, np.inf),
              ((0, 0, 0), (np.nan, 1, 0), 0.0, np.inf), ((0, 0, 0), (0, -np.inf, 1), 0.0, np.inf), ((0, 0, 0), (1e-42, 0, 0), -np.inf, np.inf),
              ((0, 0, -5), (0, 0, 1), 8.0, 2.0), ((0, 0, -5), (0.01, 0.02, 1), 1.0, 0.5)]
N_DEGENERATE = len(DEGENERATE)


@functools.lru_cache(maxsize=None)
def batch(name, n=640, seed=0):
    """the mixed batch of about 4 k rays of a mesh -> dict o, d [Q, 3], tmin, tmax [Q] (float32), want = RR.cast of it for the three culls,
    at_t / below_t = the rows whose t_max is a hit's own t / the float below it.  The degenerate rays are the last N_DEGENERATE rows."""
    v, f = mesh(name)
    rng = np.random.default_rng(seed)
    lo, hi = finite_box(v, f)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    ctr, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo)) or 1.0
    inbox = lambda k: rng.uniform(lo, hi, (k, 3))                                 # noqa: E731
    unit = lambda k: (lambda x: x / np.linalg.norm(x, axis=1, keepdims=True))(rng.standard_normal((k, 3)))   # noqa: E731
    O, D = [], []
    # from outside towards the box, unnormalised; from inside, any direction
    o = ctr + 1.5 * diag * unit(n)
    O.append(o)
    D.append((inbox(n) - o) * rng.uniform(0.2, 3.0, (n, 1)))
    O.append(inbox(n))
    D.append(unit(n))
    far = ctr + diag * unit(n // 4) * np.array([[30.0], [3000.0]]).repeat(n // 8, 0)       # where the origin's ulp is coarser than a face
    O.append(far)
    D.append(inbox(len(far)) - far)
    # one and two zero components, through points of the box
    for zeros in (1, 2):
        d = rng.standard_normal((n // 2, 3))
        for i in range(len(d)):
            d[i, rng.permutation(3)[:zeros]] = 0.0
        O.append(inbox(n // 2) - 2.0 * diag * d / np.linalg.norm(d, axis=1, keepdims=True))
        D.append(d)
    # the same with the origin exactly on a plane of the mesh's box, along an axis the ray does not move on (0 * inf in a slab product)
    d = rng.standard_normal((n // 2, 3))
    o = inbox(n // 2)
    for i in range(len(d)):
        z = rng.permutation(3)[:1 + i % 2]
        d[i, z] = 0.0
        o[i, z[0]] = (lo, hi)[i % 2][z[0]]
        o[i] -= 2.0 * diag * d[i] / np.linalg.norm(d[i])
    O.append(o)
    D.append(d)
    # aimed at vertices, edge midpoints and centroids, from outside and from inside; origins exactly on a face
    tg = targets(v, f) if len(f) else np.zeros((0, 3), F32)
    if len(tg):
        for org in (ctr + diag * np.array([0.9, -1.1, 1.3]), ctr + 0.01 * diag):
            to, td = rays_to(org, tg[rng.permutation(len(tg))[:n // 2]])
            O.append(to)
            D.append(td)
        O.append(tg[rng.permutation(len(tg))[:n // 2]])
        D.append(unit(len(O[-1])))
    o, d = np.concatenate(O).astype(F32), np.concatenate(D).astype(F32)
    Q = len(o)
    tmin, tmax = np.zeros(Q, F32), np.full(Q, np.inf, F32)
    sel = rng.permutation(Q)[:Q // 4]                                             # a range of their own for a quarter of the rays
    scale = diag / np.maximum(np.linalg.norm(d[sel].astype(np.float64), axis=1), 1e-30)
    tmin[sel] = (rng.uniform(-0.5, 2.0, len(sel)) * scale).astype(F32)
    tmax[sel] = (tmin[sel] + rng.uniform(0.0, 2.0, len(sel)) * scale).astype(F32)
    # t_max = a hit's own t (still a hit) and the float below it (a miss)
    first = RR.cast(v, f, o[:2 * n], d[:2 * n])['none']
    rows = np.nonzero(first['occluded'] & np.isfinite(first['t']))[0][:n // 2]
    at_t = np.arange(Q, Q + len(rows))
    below_t = at_t + len(rows)
    o = np.concatenate([o, o[rows], o[rows], np.array([r[0] for r in DEGENERATE], F32)])
    d = np.concatenate([d, d[rows], d[rows], np.array([r[1] for r in DEGENERATE], F32)])
    tmin = np.concatenate([tmin, np.zeros(2 * len(rows), F32), np.array([r[2] for r in DEGENERATE], F32)])
    tmax = np.concatenate([tmax, first['t'][rows], np.nextafter(first['t'][rows], F32(-np.inf)), np.array([r[3] for r in DEGENERATE], F32)])
    want = RR.cast(v, f, o, d, tmin, tmax, culls=('none', 'back', 'front'))
    return {'o': o, 'd': d, 'tmin': tmin, 'tmax': tmax, 'want': want, 'at_t': at_t, 'below_t': below_t, 'first_t': first['t'][rows],
            'first_face': first['face'][rows]}
