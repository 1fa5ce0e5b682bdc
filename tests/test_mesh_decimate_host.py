"""CPU: the C-ABI of cnerf_mesh_decimate_* (csrc/mesh_decimate.hip) up to the point where it would launch, and the NumPy restatement
(tests/qem_restatement.py) on hand-built meshes."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import qem_restatement as Q  # noqa: E402
from mesh_testlib import grid, octahedron_sphere  # noqa: E402

ROOT = os.path.dirname(HERE)
EINVAL, ENULL = -1, -2
NAMES = ["cnerf_mesh_decimate_workspace_bytes", "cnerf_mesh_decimate_init", "cnerf_mesh_decimate_round", "cnerf_mesh_decimate_emit"]


# ------------------------------------------------------------------------------------------------ C-ABI
def test_symbols_declared_bound_exported():
    from customnerf_amd import _lib
    src = open(os.path.join(ROOT, "include", "customnerf_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8


def test_workspace_bytes_grows():
    from customnerf_amd import mesh
    prev = 0
    for V, F in ((0, 0), (3, 1), (1000, 2000), (1 << 20, 1 << 21)):
        b = mesh.decimate_workspace_bytes(V, F)
        assert b > prev and b % 256 == 0
        lo = 121 * V + 12 * (V // 2 + 1) + 73 * F
        assert lo <= b <= lo + 8 * (max(V, F) // 256 + 1) + 20 * 256
        prev = b
    assert mesh.decimate_workspace_bytes(1000, 3000) > mesh.decimate_workspace_bytes(1000, 2000)
    assert mesh.decimate_workspace_bytes(2000, 2000) > mesh.decimate_workspace_bytes(1000, 2000)
    for V, F, b in ((0, 0, 1024), (3, 1, 4608), (1000, 2000, 274944), (1 << 20, 1 << 21, 286327552),
                    ((1 << 31) - 1, 0x55555555, 377308403456), (3, 0x55555555, 104555613184)):       # pinned, up to the largest accepted
        assert mesh.decimate_workspace_bytes(V, F) == b
    lib = mesh.lib
    out = C.c_uint64(0)
    wsb = lib.cnerf_mesh_decimate_workspace_bytes
    assert wsb(1 << 31, 0, C.byref(out)) == EINVAL
    assert wsb(0, 1 << 31, C.byref(out)) == EINVAL
    assert wsb(3, 0x55555556, C.byref(out)) == EINVAL                                      # edge ids 3 f + k must fit 32 bits
    assert wsb(3, 0x55555555, C.byref(out)) == 0
    assert wsb(3, 1, None) == ENULL


def test_argument_checks_reject_before_launch():
    from customnerf_amd._lib import lib
    out = C.c_uint64(0)
    assert lib.cnerf_mesh_decimate_workspace_bytes(8, 4, C.byref(out)) == 0
    wsb = out.value
    fake = 1 << 20                                   # never dereferenced: every call below is rejected first
    init, rnd, emit = lib.cnerf_mesh_decimate_init, lib.cnerf_mesh_decimate_round, lib.cnerf_mesh_decimate_emit
    assert init(fake, 1 << 31, fake, 4, fake, wsb, fake, None) == EINVAL
    assert init(fake, 8, fake, 1 << 31, fake, wsb, fake, None) == EINVAL
    assert init(None, 8, fake, 4, fake, wsb, fake, None) == ENULL                          # verts with V > 0
    assert init(fake, 8, None, 4, fake, wsb, fake, None) == ENULL                          # faces with F > 0
    assert init(fake, 8, fake, 4, None, wsb, fake, None) == ENULL
    assert init(fake, 8, fake, 4, fake, wsb, None, None) == ENULL
    assert init(fake, 8, fake, 4, fake, wsb - 1, fake, None) == EINVAL                     # short workspace
    assert init(fake, 8, fake, 4, fake + 4, wsb, fake, None) == EINVAL                     # misaligned workspace
    assert rnd(1 << 31, 4, 2, fake, wsb, fake, None) == EINVAL
    assert rnd(8, 1 << 31, 2, fake, wsb, fake, None) == EINVAL
    assert rnd(8, 4, 2, None, wsb, fake, None) == ENULL
    assert rnd(8, 4, 2, fake, wsb, None, None) == ENULL
    assert rnd(8, 4, 2, fake, wsb - 1, fake, None) == EINVAL
    assert rnd(8, 4, 2, fake + 8, wsb, fake, None) == EINVAL
    args = [None, 8, 4, fake, wsb, fake, None, fake, fake, 8, 4, None]

    def with_(i, v):
        a = list(args)
        a[i] = v
        return emit(*a)
    assert with_(1, 1 << 31) == EINVAL
    assert with_(2, 1 << 31) == EINVAL
    assert with_(3, None) == ENULL
    assert with_(5, None) == ENULL                                                         # verts_out with max_verts > 0
    assert with_(7, None) == ENULL                                                         # faces_out with max_faces > 0
    assert with_(4, wsb - 1) == EINVAL
    assert with_(3, fake + 4) == EINVAL


# ------------------------------------------------------------------------------------------------ restatement on hand meshes
def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    return v, f


def test_planar_grid_zero_costs():
    v, f = grid(8)
    st, flags = Q.init(v, f)
    assert flags == 0
    n = 8
    on_boundary = (v[:, 0] == 0) | (v[:, 0] == n) | (v[:, 1] == 0) | (v[:, 1] == n)
    for target in (100, 61, 40):
        vo, fo, _, old, rounds = Q.decimate(v, f, target)
        assert len(fo) in (target - 1, target)
        assert sum(r[2] for r in rounds) == (len(f) - len(fo)) // 2
        assert (vo[:, 2] == 0).all()                                               # every face still in the plane
        b = on_boundary[old]
        assert b.sum() == on_boundary.sum()                                        # boundary vertices kept ...
        np.testing.assert_array_equal(vo[b], v[old[b]])                            # ... and unmoved
        assert Q.check_manifold(fo) == 4 * n
        assert Q.euler(fo) == 1
        fn = np.cross(vo[fo[:, 1]] - vo[fo[:, 0]], vo[fo[:, 2]] - vo[fo[:, 0]])
        assert (fn[:, 2] > 0).all()                                                # no flip, no degenerate face
        # zero costs: the first round's keys are edge ids alone, so the cheapest edge is the smallest canonical half-edge id
        assert rounds[0][2] > 0


def test_tetrahedron_unchanged():
    v, f = tetrahedron()
    vo, fo, _, old, rounds = Q.decimate(v, f, 0)
    np.testing.assert_array_equal(fo, f)
    np.testing.assert_array_equal(old, np.arange(4))
    assert rounds == [(4, 4, 0)]


def test_flags():
    v, f = tetrahedron()
    assert Q.init(v, np.array([[0, 1, 4]]))[1] == Q.BAD_INDEX
    assert Q.init(v, np.array([[0, -1, 2]]))[1] == Q.BAD_INDEX
    assert Q.init(v, np.array([[0, 1, 2], [0, 1, 3], [1, 0, 2], [1, 0, 3]]))[1] == Q.NON_MANIFOLD   # three and more faces on (0, 1)
    assert Q.init(v, np.array([[0, 1, 2], [0, 1, 3]]))[1] == Q.NON_MANIFOLD                         # two faces with 0 -> 1
    assert Q.init(v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 3]]))[1] == Q.NON_MANIFOLD              # three faces on one edge
    assert Q.init(v, np.array([[0, 1, 1], [1, 2, 3]]))[1] == Q.REPEATED
    assert Q.init(v, f)[1] == 0


def test_sphere_keeps_euler_characteristic():
    v, f = octahedron_sphere(3)                                                    # 512 faces
    assert Q.check_manifold(f) == 0 and Q.euler(f) == 2
    for target in (300, 100, 24):
        vo, fo, _, old, rounds = Q.decimate(v, f, target)
        assert len(fo) in (target - 1, target)
        assert Q.check_manifold(fo) == 0 and Q.euler(fo) == 2
        assert len(vo) == rounds[-1][0] == len(np.unique(fo))
        np.testing.assert_array_equal(np.sort(old), old)


def test_target_at_or_above_f_returns_the_mesh():
    v, f = octahedron_sphere(1)
    v2 = np.concatenate([v, np.zeros((3, 3), np.float32)])                        # unreferenced vertices are dropped
    vo, fo, _, old, rounds = Q.decimate(v2, f, len(f))
    assert rounds == [] and np.array_equal(fo, f) and np.array_equal(vo, v) and np.array_equal(old, np.arange(len(v)))
