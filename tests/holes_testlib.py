"""Meshes with known holes that the hole-filling tests share (tests/test_mesh_holes_host.py, tests/test_gpu_mesh_holes.py).  A plain
module: neither test file imports the other."""
import numpy as np

import mesh_testlib as L


def holed_sphere():
    """octahedron_sphere(3) without face 100 and the 1-rings of vertices 0 and 1 (four faces each) -> (verts, faces, the removed face)"""
    v, f = L.octahedron_sphere(3)
    drop = (f == 0).any(1) | (f == 1).any(1)
    assert not drop[100] and drop.sum() == 8
    drop[100] = True
    return v, f[~drop], f[100]


def pinched_sphere():
    """octahedron_sphere(3) without two faces that share exactly one vertex"""
    v, f = L.octahedron_sphere(3)
    g = next(int(i) for i in range(1, len(f)) if len(set(f[0]) & set(f[i])) == 1)
    return v, np.delete(f, [0, g], axis=0)


def meshes():
    d = {name: (v, f, n) for name, v, f, n in L.decimate_meshes() if name != "jittered_sphere"}
    d["sphere"] = L.octahedron_sphere(3) + (None,)
    d["holed_sphere"] = holed_sphere()[:2] + (None,)
    d["pinched_sphere"] = pinched_sphere() + (None,)
    return d
