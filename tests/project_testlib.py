"""What the projection tests share (tests/test_mesh_project_host.py, tests/test_gpu_mesh_project.py): the sphere, thin-slab, rim,
opposed-normal and displaced-vertex cases of cnerf_mesh_bvh_project, the sphere's with the answer of tests/project_restatement.py
computed once.  A plain module, NumPy only."""
import functools

import numpy as np

import atlas_restatement as A
import project_restatement as P
import ray_testlib as T
from mesh_testlib import grid

F32 = np.float32
R_SPHERE = 64


@functools.lru_cache(maxsize=None)
def sphere():
    """the texels of an 80-face icosphere's uniform atlas (s = 9: 40 cells of 81 texels, Q = 3240, no multiple of the block) as queries
    against a 1280-face icosphere with normals = positions -> dict lv, lf (the low mesh), sv, sf (the source), x, n [Q, 3], X, Y [Q]
    (the texels' positions in the image), inradius (of the source, float64)"""
    lv, lf = T.icosphere(1)
    sv, sf = T.icosphere(3)
    x, d = A.points(lv, lf, R_SPHERE, normals=lv)
    face, _, _, X, Y = A.cell_texels(len(lf), R_SPHERE)
    assert (face >= 0).all() and len(x) == 3240
    a, b, c = (sv[sf[:, k]].astype(np.float64) for k in range(3))
    nrm = np.cross(b - a, c - a)
    inradius = float(np.abs((a * nrm).sum(1) / np.linalg.norm(nrm, axis=1)).min())      # the nearest face plane to the centre
    return {'lv': lv, 'lf': lf, 'sv': sv, 'sf': sf, 'x': x, 'n': (-d).astype(F32), 'X': X, 'Y': Y, 'inradius': inradius}


@functools.lru_cache(maxsize=None)
def sphere_want(reach, with_normals=True):
    s = sphere()
    return P.project(s['sv'], s['sf'], s['sv'] if with_normals else None, s['x'], s['n'], reach)


def slab():
    """two 4 x 4 sheets 0.05 apart, a thin wall: the top one at z = 0.05 wound towards +z (faces 0 .. 31), the bottom one at z = 0 wound
    towards -z (faces 32 .. 63)"""
    gv, gf = grid(4)
    top = gv + np.array([0, 0, 0.05], F32)
    return np.concatenate([top, gv]).astype(F32), np.concatenate([gf, gf[:, [0, 2, 1]] + len(gv)]).astype(np.int32)


def slab_queries(z, seed=11, Q=64):
    xy = np.random.default_rng(seed).uniform(0.3, 3.7, (Q, 2))
    return np.concatenate([xy, np.full((Q, 1), z)], 1).astype(F32), np.tile(np.array([[0, 0, 1]], F32), (Q, 1))


SLAB_REACH = 0.2
SLAB_HEIGHTS = ((0.07, -0.02, 2), (0.03, 0.02, 1), (0.01, 0.04, 1))             # (z of the queries, the offset to the top sheet, its kind)

RIM_X, RIM_N = np.array([[-0.1, 2.0, 0.05]], F32), np.array([[0, 0, 1]], F32)


def opposed():
    """three triangles in x = 0 wound towards +x with vertex normals that tilt (face 0: (3, 0, 4) at every vertex), that cancel at the
    barycentrics (1/4, 1/4, 1/2) (face 1: +x, -x and 0), and that are not finite (face 2); the three queries in front of them, with the
    direction (2, 0, 1) — neither the faces' normal nor +z — meet them at exactly those barycentrics, at t = 1/4 of the backward ray (every
    number here is a small dyadic fraction: the rule's arithmetic is exact) -> (verts, faces, normals, x, n)"""
    tri = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    v = np.concatenate([tri, tri + np.array([0, 2, 0], F32), tri + np.array([0, 4, 0], F32)])
    f = np.arange(9, dtype=np.int32).reshape(3, 3)
    nrm = np.array([[3, 0, 4], [3, 0, 4], [3, 0, 4], [1, 0, 0], [-1, 0, 0], [0, 0, 0], [np.nan, 0, 1], [1, 0, 0], [1, 0, 0]], F32)
    x = np.array([[0.5, 0.25, 0.75], [0.5, 2.25, 0.75], [0.5, 4.25, 0.75]], F32)
    return v, f, nrm, x, np.tile(np.array([[2, 0, 1]], F32), (3, 1))


def displaced(name, reach, seed=5):
    """queries about ray_testlib's mesh `name`, as a function of its vertex normals [V, 3] -> (x, n): the origins and directions of
    ray_testlib.DEGENERATE; the vertices moved along +- their normals by seeded amounts up to twice the reach, with those normals scaled by
    0.5 .. 2 as directions (they are not normalised, and the reach counts in their length); and, so that the closest-point rule is asked
    too, the vertices moved outwards by 0.1 .. 0.5 of the reach with a direction in the tangent plane, along which both rays leave a
    convex surface without meeting it"""
    v, _ = T.mesh(name)

    def make(normals):
        rng = np.random.default_rng(seed)
        nv = np.asarray(normals, np.float64)
        with np.errstate(all="ignore"):                                           # a vertex of zero-area faces only has no normal: a degenerate query
            nv = nv / np.linalg.norm(nv, axis=1, keepdims=True)
        amount = rng.uniform(-2.0 * reach, 2.0 * reach, (len(v), 1))
        scale = rng.uniform(0.5, 2.0, (len(v), 1))
        axis = np.eye(3)[np.argmin(np.abs(nv), 1)]
        tangent = np.cross(nv, axis)
        with np.errstate(all="ignore"):
            tangent /= np.linalg.norm(tangent, axis=1, keepdims=True)
        lift = rng.uniform(0.1, 0.5, (len(v), 1)) * reach
        x = np.concatenate([np.array([r[0] for r in T.DEGENERATE], np.float64), v + amount * scale * nv, v + lift * nv])
        n = np.concatenate([np.array([r[1] for r in T.DEGENERATE], np.float64), scale * nv, tangent])
        return x.astype(F32), n.astype(F32)
    return make
