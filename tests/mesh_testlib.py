"""What the mesh tests share (tests/test_gpu_mesh*.py, tests/test_mesh_*host.py): array <-> device helpers, lattices and mesh builders, and the
Gaussian-density model of the end-to-end tests.  A plain module: test files import what they use, and none imports another test file."""
import functools
import math

import numpy as np
import pytest
import torch

import mc_restatement as R


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


def lattice(shape, lo, hi):
    axes = [np.linspace(lo, hi, n, dtype=np.float32) for n in shape]
    return np.meshgrid(*axes, indexing="ij"), [float(a[1] - a[0]) for a in axes]


BLOBS = [(0.85, 0.0, 0.0, 0.08), (-0.8, 0.5, 0.3, 0.06), (0.1, -0.85, -0.6, 0.1), (-0.7, -0.75, 0.75, 0.07), (0.6, 0.7, -0.7, 0.05)]


def speckled_sphere(n=56):
    """(sphere-only volume, sphere + speckle volume, spacing, origin): the blobs sit >= 3 voxels away from the sphere's surface"""
    (X, Y, Z), sp = lattice((n, n, n), -1.0, 1.0)
    sphere = (0.55 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)
    vol = sphere.copy()
    for cx, cy, cz, r in BLOBS:
        vol = np.maximum(vol, (r - np.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2)).astype(np.float32))
    return sphere, vol, sp, (-1.0, -1.0, -1.0)


def grid(n):
    """planar integer grid of n x n quads in z = 0, wound counter-clockwise (normals +z)"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([i.ravel(), j.ravel(), np.zeros(i.size)], 1).astype(np.float32)
    idx = lambda a, b: a * (n + 1) + b                                             # noqa: E731
    f = []
    for a in range(n):
        for b in range(n):
            f += [[idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)], [idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)]]
    return v, np.array(f, np.int32)


def octahedron_sphere(level=2):
    """subdivided octahedron projected to the unit sphere: closed, genus 0"""
    v = [np.array(p, float) for p in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1])]
    f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int32)


def _decimate_mc_meshes():
    rng = np.random.default_rng(23)
    (X, Y, Z), sp = lattice((24, 24, 24), -1.0, 1.0)
    r = np.sqrt(X ** 2 + Y ** 2 + Z ** 2)
    vol = (0.7 - r + 0.04 * rng.standard_normal(r.shape)).astype(np.float32)                 # jittered sphere
    yield ("jittered_sphere",) + R.marching_cubes(vol, 0.0, sp, (-1.0, -1.0, -1.0))
    (X, Y, Z), sp = lattice((40, 30, 26), -1.0, 1.0)
    t1 = 0.15 - np.sqrt((np.sqrt((X + 0.45) ** 2 + Y ** 2) - 0.35) ** 2 + Z ** 2)
    t2 = 0.1 - np.sqrt((np.sqrt((X - 0.5) ** 2 + Z ** 2) - 0.3) ** 2 + Y ** 2)
    yield ("two_tori",) + R.marching_cubes(np.maximum(t1, t2).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))
    rng = np.random.default_rng(17)
    yield ("noise",) + R.marching_cubes(rng.random((16, 16, 16), dtype=np.float32), 0.55, (0.5, 0.25, 1.0), (3.0, -2.0, 0.5))
    (X, Y, Z), sp = lattice((26, 26, 20), -1.0, 1.0)
    cut = (0.8 - np.sqrt(X ** 2 + Y ** 2 + (Z + 0.5) ** 2)).astype(np.float32)               # cut open by the volume's z = -1 face
    yield ("cut_sphere",) + R.marching_cubes(cut, 0.0, sp, (-1.0, -1.0, -1.0))


@functools.lru_cache(maxsize=None)
def decimate_meshes():
    """[(name, verts, faces, normals)] of the decimation tests, which the smoothing tests reuse by index; built once"""
    return list(_decimate_mc_meshes()) + [("planar_grid",) + grid(16) + (None,)]


# ------------------------------------------------------------------------------------------------ end to end through NeRFNetwork
R_SPHERE = math.sqrt(-0.08 * math.log(math.log(10.0) / 5.0))                  # trunc_exp(5 exp(-|x|^2 / 0.08)) == 10
AABB = [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5]


@pytest.fixture
def dtype_guard():
    from customnerf_amd import tcnn
    prev = tcnn._DEFAULT_DTYPE
    yield tcnn
    tcnn.set_default_dtype(prev)


def gaussian_model(tcnn, fp16, **kw):
    from customnerf_amd import scene as sc
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    tcnn.set_default_dtype(torch.float16 if fp16 else torch.float32)
    opt = sc.make_opt(num_levels=4, n_hidden_geo=1, **kw)
    model = NeRFNetwork(opt).cuda().eval()
    with torch.no_grad():
        model.density_network.params.zero_()                                   # sigma = trunc_exp(gaussian(x)) exactly
    return model
