"""Meshes and sampling helpers that the area-proportional atlas tests share (tests/test_mesh_texture_sized_host.py on the CPU,
tests/test_gpu_mesh_texture_sized.py on the GPU).  A plain module: neither test file imports the other."""
import functools

import numpy as np

import mc_restatement as R
from mesh_testlib import lattice

f32 = np.float32
TINY = np.float32(2.0 ** -70)                                                 # its square, 2^-140, is a float32 denormal
HUGE = np.float32(2.0 ** 65)                                                  # its square overflows float32


def _triangle(rng, length):
    """three vertices of a random triangle whose longest edge is about `length`"""
    a = rng.standard_normal(3)
    u = rng.standard_normal(3)
    u /= np.linalg.norm(u)
    w = np.cross(u, rng.standard_normal(3))
    w /= np.linalg.norm(w)
    return np.stack([a, a + length * u, a + length * (0.4 * u + 0.7 * w)])


@functools.lru_cache(maxsize=None)
def hand_soup():
    """(verts, faces, normals, names): 41 faces on their own vertices with longest edges from 2^-4 to 2^6 — one face at 2^6, three a little under 2^5,
    five under 2^4, six under 2^3, the rest small — then the key edges: a longest edge of exactly 32 and of the float below 32 (a bin boundary
    and the bin under it), a zero-area face, a zero-length face, a face whose squared edge is denormal and one whose squared edge is inf.
    `names` maps the special faces to their index."""
    rng = np.random.default_rng(41)
    lengths = [2.0 ** 6] + [2.0 ** 5 * 0.8] * 3 + [2.0 ** 4 * 0.85] * 5 + [2.0 ** 3 * 0.9] * 6 + list(2.0 ** rng.uniform(-4, 1, 20))
    tris = [_triangle(rng, l) for l in lengths]
    names = {}

    def add(name, t):
        names[name] = len(tris)
        tris.append(np.asarray(t, np.float64))
    below = float(np.nextafter(f32(32), f32(0)))
    add("boundary", [[1, 1, 1], [33, 1, 1], [17, 2, 1]])
    add("below_boundary", [[0, 0, 0], [below, 0, 0], [16, 1, 0]])
    add("zero_area", [[0, 0, 0], [1, 1, 1], [2, 2, 2]])
    add("zero_length", [[3, 4, 5]] * 3)
    add("denormal", [[0, 0, 0], [float(TINY), 0, 0], [0, float(TINY), 0]])
    add("overflow", [[0, 0, 0], [float(HUGE), 0, 0], [0, 1, 0]])
    v = np.concatenate(tris).astype(f32)
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    f = f[rng.permutation(len(f))]                                             # classes interleave in face order
    names = {k: int(np.nonzero(f[:, 0] == 3 * i)[0][0]) for k, i in names.items()}
    nrm = rng.standard_normal(v.shape).astype(f32)
    return v, f, nrm, names


@functools.lru_cache(maxsize=None)
def random_soup(F=5001, sigma=0.8, seed=7):
    """F faces on their own vertices whose longest edges are log-normal"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([_triangle(rng, l) for l in np.exp(sigma * rng.standard_normal(F))]).astype(f32)
    return v, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


@functools.lru_cache(maxsize=None)
def sphere_mesh(n=40, r=0.9):
    (X, Y, Z), sp = lattice((n, n, n), -1.0, 1.0)
    return R.marching_cubes((r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))


@functools.lru_cache(maxsize=None)
def torus_mesh():
    (X, Y, Z), sp = lattice((48, 44, 36), -1.0, 1.0)
    q = np.sqrt(X ** 2 + Y ** 2) - 0.6
    return R.marching_cubes((0.25 - np.sqrt(q ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))


def triangle_samples(c, rng, k_edge=9, k_in=40):
    """points of the triangle with corners c [3, 2] (texel coordinates): corners, points along every edge, random interior points"""
    pts = [c]
    t = np.arange(1, k_edge)[:, None] / k_edge
    for a, b in ((0, 1), (1, 2), (2, 0)):
        pts.append(c[a] + t * (c[b] - c[a]))
    w = rng.random((k_in, 3)) + 1e-3
    w /= w.sum(1, keepdims=True)
    pts.append(w @ c)
    return np.concatenate(pts)


def bilinear_footprint(p):
    """the texels with a nonzero bilinear weight at the points p [N, 2] (texel centres at integer coordinates) -> (X, Y) int64 arrays"""
    x0, y0 = np.floor(p[:, 0]).astype(np.int64), np.floor(p[:, 1]).astype(np.int64)
    fx, fy = p[:, 0] > x0, p[:, 1] > y0
    X, Y = [], []
    for dx, dy, m in ((0, 0, np.ones(len(p), bool)), (1, 0, fx), (0, 1, fy), (1, 1, fx & fy)):
        X.append(x0[m] + dx)
        Y.append(y0[m] + dy)
    return np.concatenate(X), np.concatenate(Y)
