"""What the winding-number tests share (tests/test_mesh_winding_host.py, tests/test_gpu_mesh_winding.py, tests/test_gpu_mesh_remesh.py): the
fixtures, each one's ~2000 query points and, computed once per fixture, the reference (the exact float64 sum) and the restated tree,
moments and walks of tests/winding_restatement.py.  A plain module, NumPy only."""
import functools

import numpy as np

import winding_restatement as W
from bvh_restatement import participating
from holes_testlib import holed_sphere
from ray_testlib import _soup, finite_box, icosphere, mc_torus

F32 = np.float32
BAND = 0.25                                                                       # |w - 0.5| <= BAND: where `contains` is not asked


def _cat(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs).astype(F32), np.concatenate(fs).astype(np.int32)


def two_spheres(level=2):
    """two unit icospheres whose centres are 0.8 radii apart along x"""
    v, f = icosphere(level)
    return _cat((v - F32([0.4, 0, 0]), f), (v + F32([0.4, 0, 0]), f))


def bad_faces():
    """icosphere(2) and two faces that take no part: one with an index outside [0, V), one at a NaN vertex"""
    v, f = icosphere(2)
    v = np.concatenate([v, np.array([[np.nan, 0.0, 0.0]], F32)])
    return v, np.concatenate([f[:100], np.array([[0, 1, len(v)]], np.int32), f[100:], np.array([[2, len(v) - 1, 3]], np.int32)])


def _fixtures():
    v, f = icosphere(2)
    yield "icosphere", v, f, True
    yield ("torus",) + mc_torus() + (True,)
    yield ("holed_sphere",) + holed_sphere()[:2] + (False,)
    yield ("nested",) + _cat((v, f), (F32(0.5) * v, f)) + (True,)
    yield "inward", v, f[:, ::-1].copy(), True
    yield ("two_spheres",) + two_spheres() + (True,)
    yield ("soup",) + _soup(40, 7) + (False,)
    yield ("bad_faces",) + bad_faces() + (True,)                                   # closed: the faces that take part are icosphere(2)
    yield "empty", v, np.zeros((0, 3), np.int32), True


FIXTURES = {name: (v, f, closed) for name, v, f, closed in _fixtures()}
NAMES = list(FIXTURES)
N_LATTICE = 11 ** 3


# On a surface w is 0.5 (a closed mesh) or jumps from about -0.5 to about 0.5 (an open one), so the queries ON the surface, and on an open
# mesh those just off it, fall into the band whatever the code does: a few of them are enough.  The soup is forty faces that are all open,
# so it gets fewer of both and a lattice over 3 x its box, which its faces cross less densely (what condition (c) of tests/test_mesh_winding_host.py asked for).
QUERY_ARGS = {"soup": dict(n_near=4, n_on=2, span=3.0)}


def queries(v, f, seed=0, n_near=240, n_on=8, span=1.5):
    """-> (points [Q, 3] float32, diag): an 11^3 lattice over `span` x the box (the first N_LATTICE rows), points 1e-3 and 1e-5 diagonals off
    the surface on both sides along the normals of n_near faces, points thousands of diagonals away, n_on vertices and n_on face centroids
    themselves, and three points that are not finite (the last rows)"""
    rng = np.random.default_rng(seed)
    lo, hi = (t.astype(np.float64) for t in finite_box(v, f))
    ctr, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo)) or 1.0
    half = 0.5 * span * np.maximum(hi - lo, 1e-3 * diag)
    ax = [np.linspace(ctr[a] - half[a], ctr[a] + half[a], 11) for a in range(3)]
    P = [np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)]
    ok, _ = participating(v, f)
    g = np.asarray(f, np.int64)[ok]
    if len(g):
        pick = g[rng.permutation(len(g))[:max(n_near, n_on)]]
        a, b, c = (v[pick[:, k]].astype(np.float64) for k in range(3))
        cen, n = (a + b + c) / 3.0, np.cross(b - a, c - a)
        keep = np.linalg.norm(n, axis=1) > 0
        cen, n = cen[keep], n[keep] / np.linalg.norm(n[keep], axis=1, keepdims=True)
        for s, m in ((1e-3, n_near), (-1e-3, n_near), (1e-5, n_near // 2), (-1e-5, n_near // 2)):
            P.append(cen[:m] + s * diag * n[:m])
        P.append(v[np.unique(g)[:n_on]].astype(np.float64))
        P.append(cen[:n_on])
    u = rng.standard_normal((96, 3))
    P.append(ctr + diag * rng.uniform(1000.0, 5000.0, (96, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True))
    P.append(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]))
    return np.concatenate(P).astype(F32), diag


def surface_distance(v, f, q):
    """the unsigned distance from each query to the faces that take part, float64 (inf without faces or for a non-finite query)"""
    from bvh_restatement import closest64
    ok, _ = participating(v, f)
    d = np.full(len(q), np.inf)
    fin = np.isfinite(q).all(1)
    if ok.any():
        d[fin] = np.sqrt(closest64(v, f, q[fin])['dist2'])
    return d


@functools.lru_cache(maxsize=None)
def case(name):
    """everything a test asks of a fixture, computed once: v, f, closed, q, diag, dist (to the surface, float64), exact (the reference),
    tree, mom (the restated moments), w2 / acc2 / tri2 (the float32 walk at beta = 2), winf / triinf (the float32 walk at beta = inf),
    w2_64 (the float64 walk at beta = 2), off (the rows at least 1e-6 diagonals off the surface), clear (the rows outside the band)"""
    v, f, closed = FIXTURES[name]
    q, diag = queries(v, f, **QUERY_ARGS.get(name, {}))
    c = {'v': v, 'f': f, 'closed': closed, 'q': q, 'diag': diag}
    c['dist'] = surface_distance(v, f, q)
    c['exact'] = W.exact(v, f, q)
    c['tree'] = W.tree(v, f)
    c['mom'] = W.moments(c['tree'])
    c['w2'], c['acc2'], c['tri2'] = W.walk(c['tree'], c['mom'], q, 2.0)
    c['winf'], accinf, c['triinf'] = W.walk(c['tree'], c['mom'], q, np.inf)
    assert not accinf.any()
    c['w2_64'] = W.walk(c['tree'], c['mom'], q, 2.0, np.float64)[0]
    c['off'] = c['dist'] >= 1e-6 * diag
    c['clear'] = np.abs(c['exact'] - 0.5) > BAND
    return c
