"""CPU: the C-ABI of cnerf_mesh_components_* / cnerf_mesh_cluster_* (csrc/mesh_clean.hip) up to the point where it would launch, and the
NumPy restatement (tests/mesh_clean_restatement.py) on hand-built meshes."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_clean_restatement as MC  # noqa: E402

ROOT = os.path.dirname(HERE)
EINVAL, ENULL = -1, -2
NAMES = ["cnerf_mesh_components_workspace_bytes", "cnerf_mesh_components_count", "cnerf_mesh_components_emit",
         "cnerf_mesh_cluster_workspace_bytes", "cnerf_mesh_cluster_count", "cnerf_mesh_cluster_emit"]


# ------------------------------------------------------------------------------------------------ C-ABI
def test_symbols_declared_and_bound():
    from customnerf_amd import _lib
    src = open(os.path.join(ROOT, "include", "customnerf_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8


def grid3(*g):
    return (C.c_uint32 * 3)(*g)


def test_workspace_bytes():
    from customnerf_amd import mesh
    for V, F in ((0, 0), (3, 1), (1000, 2000), (1 << 20, 1 << 21)):
        b = mesh.components_workspace_bytes(V, F)
        assert 12 * V <= b <= 12 * V + 8 * (max(V, F) // 256 + 1) + 5 * 256
    for V, F, g in ((0, 0, (1, 1, 1)), (100, 200, (4, 5, 6)), (1 << 20, 1 << 21, (128, 128, 128))):
        G, K = g[0] * g[1] * g[2], min(V, g[0] * g[1] * g[2])
        b = mesh.cluster_workspace_bytes(V, F, g)
        assert 4 * V + 5 * G + 12 * F + 132 * K <= b <= 4 * V + 5 * G + 20 * F + 132 * K + 8 * (max(G, F) // 256 + 1) + 10 * 256 + 64 * 4
    M = (1 << 31) - 1                                                                      # pinned sizes, up to the largest V and F accepted
    for V, F, b in ((0, 0, 512), (3, 1, 1280), (1000, 2000, 12800), (1 << 20, 1 << 21, 12648704), (M, M, 25836912896), (5, M, 67109888)):
        assert mesh.components_workspace_bytes(V, F) == b
    for V, F, g, b in ((0, 0, (1, 1, 1), 1280), (3, 1, (1, 1, 1), 2304), (100, 200, (4, 5, 6), 18176), (1000, 2000, (7, 1, 13), 42240),
                       (1 << 20, 1 << 21, (128, 128, 128), 178323712), (824914, 1670112, (128, 128, 128), 146198016),
                       (M, M, (1024, 1024, 2047), 328488452352), (3, 1, (1024, 1024, 2047), 10799253248)):
        assert mesh.cluster_workspace_bytes(V, F, g) == b
    lib = mesh.lib
    out = C.c_uint64(0)
    assert lib.cnerf_mesh_components_workspace_bytes(1 << 31, 0, C.byref(out)) == EINVAL
    assert lib.cnerf_mesh_components_workspace_bytes(0, 1 << 31, C.byref(out)) == EINVAL
    assert lib.cnerf_mesh_components_workspace_bytes(3, 1, None) == ENULL
    assert lib.cnerf_mesh_cluster_workspace_bytes(3, 1, grid3(1024, 1024, 2048), C.byref(out)) == EINVAL    # 2^31 cells
    assert lib.cnerf_mesh_cluster_workspace_bytes(3, 1, grid3(1024, 1024, 2047), C.byref(out)) == 0
    assert lib.cnerf_mesh_cluster_workspace_bytes(3, 1, grid3(0, 4, 4), C.byref(out)) == EINVAL
    assert lib.cnerf_mesh_cluster_workspace_bytes(3, 1, None, C.byref(out)) == ENULL
    assert lib.cnerf_mesh_cluster_workspace_bytes(1 << 31, 1, grid3(2, 2, 2), C.byref(out)) == EINVAL


def test_components_argument_checks_reject_before_launch():
    from customnerf_amd._lib import lib
    out = C.c_uint64(0)
    assert lib.cnerf_mesh_components_workspace_bytes(8, 4, C.byref(out)) == 0
    wsb = out.value
    fake = 1 << 20                                   # never dereferenced: every call below is rejected first
    count, emit = lib.cnerf_mesh_components_count, lib.cnerf_mesh_components_emit
    assert count(fake, 1 << 31, 4, 1, 0, fake, wsb, fake, None) == EINVAL
    assert count(fake, 8, 1 << 31, 1, 0, fake, wsb, fake, None) == EINVAL
    assert count(None, 8, 4, 1, 0, fake, wsb, fake, None) == ENULL                    # faces with F > 0
    assert count(fake, 8, 4, 1, 0, None, wsb, fake, None) == ENULL
    assert count(fake, 8, 4, 1, 0, fake, wsb, None, None) == ENULL
    assert count(fake, 8, 4, 1, 0, fake, wsb - 1, fake, None) == EINVAL               # short workspace
    assert count(fake, 8, 4, 1, 0, fake + 4, wsb, fake, None) == EINVAL               # misaligned workspace
    args = [fake, None, 8, fake, 4, 1, 0, fake, wsb, fake, None, fake, None, 8, 4, None]
    assert emit(*args[:2], 1 << 31, *args[3:]) == EINVAL

    def with_(i, v):
        a = list(args)
        a[i] = v
        return emit(*a)
    assert with_(0, None) == ENULL                                                     # verts with V > 0
    assert with_(3, None) == ENULL                                                     # faces with F > 0
    assert with_(7, None) == ENULL
    assert with_(9, None) == ENULL                                                     # verts_out with max_verts > 0
    assert with_(11, None) == ENULL                                                    # faces_out with max_faces > 0
    assert with_(8, wsb - 1) == EINVAL
    assert with_(7, fake + 8) == EINVAL


def test_cluster_argument_checks_reject_before_launch():
    from customnerf_amd._lib import lib
    out = C.c_uint64(0)
    g = grid3(4, 4, 4)
    assert lib.cnerf_mesh_cluster_workspace_bytes(8, 4, g, C.byref(out)) == 0
    wsb = out.value
    fake = 1 << 20
    o3, c3 = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    count, emit = lib.cnerf_mesh_cluster_count, lib.cnerf_mesh_cluster_emit
    base = [fake, 8, fake, 4, o3, c3, g, fake, wsb, fake, None]

    def cnt(i, v):
        a = list(base)
        a[i] = v
        return count(*a)
    assert cnt(0, None) == ENULL and cnt(2, None) == ENULL and cnt(4, None) == ENULL and cnt(5, None) == ENULL
    assert cnt(6, None) == ENULL and cnt(7, None) == ENULL and cnt(9, None) == ENULL
    assert cnt(1, 1 << 31) == EINVAL and cnt(3, 1 << 31) == EINVAL
    assert cnt(8, wsb - 1) == EINVAL and cnt(7, fake + 4) == EINVAL
    assert cnt(6, grid3(1 << 11, 1 << 10, 1 << 10)) == EINVAL                         # 2^31 cells
    assert cnt(6, grid3(4, 0, 4)) == EINVAL
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, float("inf")), (1, float("nan"), 1)):
        assert cnt(5, (C.c_float * 3)(*bad)) == EINVAL                                 # cell finite and > 0
    assert cnt(4, (C.c_float * 3)(0, float("nan"), 0)) == EINVAL                      # origin finite
    eb = [fake, None, 8, fake, 4, o3, c3, g, fake, wsb, fake, None, fake, 8, 4, None]

    def em(i, v):
        a = list(eb)
        a[i] = v
        return emit(*a)
    assert em(0, None) == ENULL and em(3, None) == ENULL and em(5, None) == ENULL and em(6, None) == ENULL and em(8, None) == ENULL
    assert em(10, None) == ENULL and em(12, None) == ENULL
    assert em(9, wsb - 1) == EINVAL and em(7, grid3(1 << 11, 1 << 10, 1 << 10)) == EINVAL


# ------------------------------------------------------------------------------------------------ restatement
def bfs_labels(faces, V):
    adj = [[] for _ in range(V)]
    for f in faces:
        for a in f:
            for b in f:
                adj[a].append(b)
    lab = [-1] * V
    for s in range(V):
        if lab[s] >= 0:
            continue
        stack, comp = [s], [s]
        lab[s] = s
        while stack:
            x = stack.pop()
            for y in adj[x]:
                if lab[y] < 0:
                    lab[y] = s
                    stack.append(y)
                    comp.append(y)
    return np.array(lab)


def test_labels_match_bfs():
    rng = np.random.default_rng(5)
    for V, F in ((1, 0), (50, 20), (300, 150), (200, 400)):
        f = rng.integers(0, V, (F, 3))
        np.testing.assert_array_equal(MC.labels(f, V), bfs_labels(f, V))


def disjoint_triangles():
    v = np.arange(3 * 12, dtype=np.float32).reshape(-1, 3)
    f = np.array([[0, 1, 2], [3, 4, 5], [5, 6, 7], [8, 9, 10], [10, 9, 11]], dtype=np.int32)
    return v, f


def test_components_disjoint_and_unreferenced():
    v, f = disjoint_triangles()                      # components {0,1,2}: 1 face, {3..7}: 2, {8..11}: 2
    vo, fo, no, old = MC.components(v, f, min_faces=2)
    np.testing.assert_array_equal(old, np.arange(3, 12))
    np.testing.assert_array_equal(fo, f[1:] - 3)
    np.testing.assert_array_equal(vo, v[3:12])
    assert no is None
    vo, fo, _, old = MC.components(v, f, largest=True)                               # tie 2 vs 2: the smaller label (3)
    np.testing.assert_array_equal(old, np.arange(3, 8))
    np.testing.assert_array_equal(fo, [[0, 1, 2], [2, 3, 4]])
    v2 = np.concatenate([v, np.ones((3, 3), np.float32)])                            # three unreferenced vertices
    n2 = np.arange(v2.size, dtype=np.float32).reshape(-1, 3)
    vo, fo, no, old = MC.components(v2, f, normals=n2, min_faces=0)
    assert len(vo) == len(v2) and np.array_equal(fo, f) and np.array_equal(no, n2)  # identity
    vo, fo, no, old = MC.components(v2, f, normals=n2, min_faces=1)
    assert len(vo) == 12 and np.array_equal(old, np.arange(12)) and np.array_equal(no, n2[:12])
    with pytest.raises(ValueError):
        MC.components(v, np.array([[0, 1, 12]]))


def test_components_empty():
    vo, fo, no, old = MC.components(np.zeros((0, 3)), np.zeros((0, 3)), largest=True)
    assert vo.shape == (0, 3) and fo.shape == (0, 3) and old.shape == (0,)
    vo, fo, _, old = MC.components(np.zeros((4, 3)), np.zeros((0, 3)), largest=True)
    assert len(vo) == 0 and len(old) == 0                                           # 0-face components only
    vo, fo, _, old = MC.components(np.zeros((4, 3)), np.zeros((0, 3)), min_faces=0)
    assert len(vo) == 4


def test_cells_formula_and_clamp():
    v = np.array([[0.0, 0.0, 0.0], [0.999999, 1.0, 2.5], [-5, 100, np.nan], [3.0, 3.0, 3.0]], dtype=np.float32)
    c = MC.cells(v, (0, 0, 0), (1, 1, 1), (3, 3, 3))
    np.testing.assert_array_equal(c, [[0, 0, 0], [0, 1, 2], [0, 2, 0], [2, 2, 2]])


def test_cluster_dedup_and_degenerate():
    # a strip of 4 unit cells along x; vertices near the cell centres, two per cell
    v = np.array([[0.2, 0.5, 0.5], [0.7, 0.5, 0.5], [1.5, 0.5, 0.5], [1.6, 0.6, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5]], dtype=np.float32)
    f = np.array([[0, 2, 4],            # clusters (0, 1, 2): survives
                  [1, 3, 4],            # same triple: dropped (first occurrence kept)
                  [4, 3, 0],            # same unordered triple, other winding: dropped
                  [0, 1, 2],            # clusters (0, 0, 1): collapsed
                  [2, 4, 5],            # (1, 2, 3): survives
                  [1, 1, 5]], dtype=np.int32)   # zero area, (0, 0, 3): collapsed
    vo, fo, _, _ = MC.cluster(v, f, (0, 0, 0), (1, 1, 1), (4, 1, 1))
    np.testing.assert_array_equal(fo, [[0, 1, 2], [1, 2, 3]])
    assert vo.shape == (4, 3)
    for k in range(4):                                                               # clamped to its cell
        assert k <= vo[k, 0] <= k + 1 and 0 <= vo[k, 1] <= 1 and 0 <= vo[k, 2] <= 1


def test_cluster_single_cell_mean_and_plane():
    # one cell, a flat patch in z = 0.3: A has rank 1, so x keeps the mean in x, y and moves z onto the plane
    rng = np.random.default_rng(2)
    xy = rng.random((30, 2)).astype(np.float32) * 0.8 + 0.1
    z = np.full((30, 1), 0.3, np.float32) + rng.standard_normal((30, 1)).astype(np.float32) * 1e-3
    v = np.concatenate([xy, z], 1)
    f = np.array([[i, i + 1, i + 2] for i in range(28)], dtype=np.int32)
    nrm = np.tile(np.array([[0, 0, 2.0]], np.float32), (30, 1))
    vo, fo, no, flagged = MC.cluster(v, f, (0, 0, 0), (1, 1, 1), (1, 1, 1), normals=nrm)
    assert len(vo) == 1 and len(fo) == 0 and not flagged.any()
    np.testing.assert_allclose(vo[0, :2], v[:, :2].astype(np.float64).mean(0), atol=1e-5)
    assert abs(vo[0, 2] - 0.3) < 3e-3
    np.testing.assert_allclose(no, [[0, 0, 1]], atol=1e-7)


def test_cluster_empty():
    vo, fo, no, flagged = MC.cluster(np.zeros((0, 3)), np.zeros((0, 3)), (0, 0, 0), (1, 1, 1), (1, 1, 1))
    assert vo.shape == (0, 3) and fo.shape == (0, 3) and len(flagged) == 0
    with pytest.raises(ValueError):
        MC.cluster(np.zeros((2, 3)), np.array([[0, 1, 2]]), (0, 0, 0), (1, 1, 1), (1, 1, 1))


def test_default_grid_covers_bbox():
    rng = np.random.default_rng(9)
    v = (rng.random((500, 3)) * [3.0, 1.0, 0.25] - 1).astype(np.float32)
    o, c, g = MC.default_grid(v, 0.1)
    cc = MC.cells(v, o, c, g)
    assert (cc.max(0) == np.array(g) - 1).all() and (cc.min(0) == 0).all()
    q = np.floor((v - o) / c)
    assert (q <= np.array(g) - 1).all()                                              # no vertex needs the clamp
