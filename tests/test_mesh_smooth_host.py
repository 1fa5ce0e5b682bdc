"""CPU: the C-ABI of cnerf_mesh_smooth_* (csrc/mesh_smooth.hip) up to the point where it would launch, and the NumPy restatement
(tests/smooth_restatement.py) against an independent dense formulation and on hand-built meshes."""
import ctypes as C
import os
import re
import sys
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mc_restatement as R  # noqa: E402
import smooth_restatement as S  # noqa: E402
from mesh_testlib import grid, lattice, octahedron_sphere  # noqa: E402

ROOT = os.path.dirname(HERE)
EINVAL, ENULL = -1, -2
NAMES = ["cnerf_mesh_smooth_workspace_bytes", "cnerf_mesh_smooth_init", "cnerf_mesh_smooth_steps", "cnerf_mesh_smooth_normals"]


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
        b = mesh.smooth_workspace_bytes(V, F)
        assert b > prev and b % 256 == 0
        lo = 48 * V + 36 * F
        assert lo <= b <= lo + 8 * (V // 256 + 1) + 12 * 256
        prev = b
    assert mesh.smooth_workspace_bytes(1000, 3000) > mesh.smooth_workspace_bytes(1000, 2000)
    assert mesh.smooth_workspace_bytes(2000, 2000) > mesh.smooth_workspace_bytes(1000, 2000)
    for V, F, b in ((0, 0, 512), (3, 1, 2816), (1000, 2000, 121344), (1 << 20, 1 << 21, 125862144),
                    ((1 << 31) - 1, 0x2AAAAAAA, 128916128000), (3, 0x2AAAAAAA, 25769806080)):         # pinned, up to the largest accepted
        assert mesh.smooth_workspace_bytes(V, F) == b
    lib = mesh.lib
    out = C.c_uint64(0)
    wsb = lib.cnerf_mesh_smooth_workspace_bytes
    assert wsb(1 << 31, 0, C.byref(out)) == EINVAL
    assert wsb(3, 0x2AAAAAAB, C.byref(out)) == EINVAL                                      # 6 F records must fit 32 bits
    assert wsb(3, 0x2AAAAAAA, C.byref(out)) == 0
    assert wsb(3, 1, None) == ENULL


def test_argument_checks_reject_before_launch():
    from customnerf_amd._lib import lib
    out = C.c_uint64(0)
    assert lib.cnerf_mesh_smooth_workspace_bytes(8, 4, C.byref(out)) == 0
    wsb = out.value
    fake = 1 << 20                                   # never dereferenced: every call below is rejected first
    init, steps, nrm = lib.cnerf_mesh_smooth_init, lib.cnerf_mesh_smooth_steps, lib.cnerf_mesh_smooth_normals
    assert init(fake, 1 << 31, 4, fake, wsb, fake, None) == EINVAL
    assert init(fake, 8, 0x2AAAAAAB, fake, wsb, fake, None) == EINVAL
    assert init(None, 8, 4, fake, wsb, fake, None) == ENULL                                # faces with F > 0
    assert init(fake, 8, 4, None, wsb, fake, None) == ENULL
    assert init(fake, 8, 4, fake, wsb, None, None) == ENULL
    assert init(fake, 8, 4, fake, wsb - 1, fake, None) == EINVAL                           # short workspace
    assert init(fake, 8, 4, fake + 4, wsb, fake, None) == EINVAL                           # misaligned workspace
    assert steps(fake, 8, 4, 3, 0.5, -0.53, 1, fake, wsb - 1, fake, None) == EINVAL
    assert steps(fake, 8, 4, 3, float("nan"), -0.53, 1, fake, wsb, fake, None) == EINVAL
    assert steps(fake, 8, 4, 3, 0.5, float("-inf"), 1, fake, wsb, fake, None) == EINVAL
    assert steps(None, 8, 4, 3, 0.5, -0.53, 1, fake, wsb, fake, None) == ENULL
    assert steps(fake, 8, 4, 3, 0.5, -0.53, 1, fake, wsb, None, None) == ENULL
    assert steps(fake, 8, 4, 3, 0.5, -0.53, 1, None, wsb, fake, None) == ENULL
    assert nrm(fake, None, 8, fake, 4, fake, wsb, None, None) == ENULL
    assert nrm(None, None, 8, fake, 4, fake, wsb, fake, None) == ENULL
    assert nrm(fake, None, 8, None, 4, fake, wsb, fake, None) == ENULL
    assert nrm(fake, None, 8, fake, 0x2AAAAAAB, fake, wsb, fake, None) == EINVAL
    assert nrm(fake, None, 8, fake, 4, fake + 8, wsb, fake, None) == EINVAL


# ------------------------------------------------------------------------------------------------ restatement
def edge_faces(faces):
    """independent count: undirected edge -> number of faces holding it (a face counts each of its distinct edges once)"""
    c = Counter()
    for t in np.asarray(faces).reshape(-1, 3).tolist():
        c.update({(min(a, b), max(a, b)) for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])) if a != b})
    return c


def expected_lists(faces, V):
    ec = edge_faces(faces)
    nbr = [set() for _ in range(V)]
    bnd = np.zeros(V, bool)
    for (a, b), k in ec.items():
        nbr[a].add(b)
        nbr[b].add(a)
        if k == 1:
            bnd[a] = bnd[b] = True
    return [sorted(s) for s in nbr], bnd


def check_lists(faces, V):
    L = S.lists(faces, V)
    nbr, bnd = expected_lists(faces, V)
    for v in range(V):
        assert L["nbr"][v, :L["count"][v]].tolist() == nbr[v], v
    np.testing.assert_array_equal(L["boundary"], bnd)
    return L


def dense_step(P, faces, s, pinned):
    """x' = x + s (D^-1 A - I) x in float64 from the adjacency matrix, pinned rows unchanged"""
    V = len(P)
    A = np.zeros((V, V))
    for a, b in edge_faces(faces):
        A[a, b] = A[b, a] = 1.0
    d = A.sum(1)
    M = np.zeros((V, V))
    has = d > 0
    M[has] = A[has] / d[has, None] - np.eye(V)[has]
    M[pinned] = 0.0
    return P + s * (M @ P)


def mc_mesh(kind):
    if kind == "cut_sphere":
        (X, Y, Z), sp = lattice((26, 26, 20), -1.0, 1.0)
        vol = (0.8 - np.sqrt(X ** 2 + Y ** 2 + (Z + 0.5) ** 2)).astype(np.float32)      # cut open by the volume's z = -1 face
    else:
        (X, Y, Z), sp = lattice((16, 16, 16), -1.0, 1.0)
        vol = (0.6 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)
    return R.marching_cubes(vol, 0.0, sp, (-1.0, -1.0, -1.0))


def test_restatement_matches_dense_formulation():
    rng = np.random.default_rng(3)
    v, f = grid(6)
    v = v + rng.normal(0, 0.2, v.shape).astype(np.float32)
    meshes = [(v, f), mc_mesh("cut_sphere")[:2], octahedron_sphere(2)]
    for v, f in meshes:
        v = np.asarray(v, np.float32)
        L = S.lists(f, len(v))
        for s, pin in ((0.5, True), (-0.53, True), (0.9, False), (-1.0, False)):
            pinned = (L["count"] == 0) | (L["boundary"] if pin else False)
            got = S.step(v, L, s, pin).astype(np.float64)
            want = dense_step(v.astype(np.float64), f, s, pinned)
            scale = max(1.0, float(np.abs(v).max()))
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 * scale)
            np.testing.assert_array_equal(got[pinned], v[pinned])


def test_grid_patch_boundary():
    n = 6
    v, f = grid(n)
    L = check_lists(f, len(v))
    border = (v[:, 0] == 0) | (v[:, 0] == n) | (v[:, 1] == 0) | (v[:, 1] == n)
    np.testing.assert_array_equal(L["boundary"], border)
    vo, no = S.smooth(v, f, 5)
    np.testing.assert_array_equal(vo, v)                          # a planar regular grid is a fixed point of uniform smoothing
    assert (no == np.array([0, 0, 1], np.float32)).all()


def test_cut_sphere_boundary_is_the_cut():
    v, f, _ = mc_mesh("cut_sphere")
    L = check_lists(f, len(v))
    np.testing.assert_array_equal(L["boundary"], v[:, 2] == -1.0)
    assert L["boundary"].sum() > 20
    vo, _ = S.smooth(v, f, 10)
    b = L["boundary"]
    np.testing.assert_array_equal(vo[b], v[b])
    assert (vo[~b] != v[~b]).any(axis=1).mean() > 0.9
    vu, _ = S.smooth(v, f, 10, pin_boundary=False)
    assert (vu[b] != v[b]).any(axis=1).all()


def test_non_manifold_fan_and_bowtie():
    ring = lambda c, ids: [[c, ids[i], ids[(i + 1) % len(ids)]] for i in range(len(ids))]        # noqa: E731
    bowtie = np.array(ring(0, [1, 2, 3, 4, 5]) + ring(0, [6, 7, 8, 9, 10]), np.int32)          # two closed fans on one vertex
    L = check_lists(bowtie, 11)
    assert not L["boundary"][0] and L["boundary"][1:].all() and L["count"][0] == 10
    book = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)                                # three faces on the edge (0, 1)
    L = check_lists(book, 6)                                                                   # vertex 5 unreferenced
    assert L["boundary"][:5].all() and L["count"][5] == 0 and not L["boundary"][5]
    fin = np.array(ring(0, [1, 2, 3, 4, 5, 6]) + [[0, 1, 7]], np.int32)                        # a fin on a spoke of a closed fan
    L = check_lists(fin, 8)
    assert L["boundary"].all()
    v = np.random.default_rng(1).random((11, 3), dtype=np.float32)
    vo, _ = S.smooth(v, bowtie, 1, 0.5, 0.0)
    np.testing.assert_array_equal(vo[1:], v[1:])
    m = v[1:].sum(0, dtype=np.float64) / 10
    np.testing.assert_allclose(vo[0], v[0] + 0.5 * (m - v[0]), rtol=0, atol=1e-6)


def test_repeated_index_faces():
    f = np.array([[0, 1, 2], [2, 1, 3], [0, 0, 3], [3, 3, 3], [4, 4, 4]], np.int32)
    L = check_lists(f, 6)
    assert L["nbr"][0, :L["count"][0]].tolist() == [1, 2, 3]
    assert L["nbr"][4, :L["count"][4]].tolist() == [] and L["count"][4] == 0     # a face (4, 4, 4) adds no edge ...
    assert L["flist"][4, :L["fcount"][4]].tolist() == [4]                         # ... but it holds the vertex once
    assert L["flist"][3, :L["fcount"][3]].tolist() == [1, 2, 3]
    assert L["flist"][0, :L["fcount"][0]].tolist() == [0, 2]
    v = np.random.default_rng(2).random((6, 3), dtype=np.float32)
    n_in = np.tile(np.array([[0.6, 0.0, 0.8]], np.float32), (6, 1))
    n = S.vertex_normals(v, f, n_in)
    np.testing.assert_array_equal(n[4], n_in[4])                                    # zero-area faces only: the input normal
    np.testing.assert_array_equal(n[5], n_in[5])                                    # unreferenced: the input normal
    assert (S.vertex_normals(v, f)[[4, 5]] == 0).all()
    assert abs(np.linalg.norm(n[0].astype(np.float64)) - 1) < 1e-6


def test_bad_index_flag():
    assert S.lists(np.array([[0, 1, 3]]), 3)["flags"] == S.BAD_INDEX
    assert S.lists(np.array([[0, -1, 2]]), 3)["flags"] == S.BAD_INDEX
    assert S.lists(np.array([[0, 1, 2]]), 3)["flags"] == 0


def test_normals_area_weighted():
    v, f = octahedron_sphere(2)
    n = S.vertex_normals(v, f)
    c = S.face_normals(v, f).astype(np.float64)
    want = np.zeros((len(v), 3))
    for k in range(3):
        np.add.at(want, f[:, k], c)
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    np.testing.assert_allclose(n, want, rtol=0, atol=1e-6)
    assert ((n * v).sum(1) > 0.95).all()


def test_taubin_keeps_volume_laplacian_shrinks():
    # the numbers the GPU test's thresholds come from (test_gpu_mesh_smooth.noisy_sphere: 48^3 marching-cubes sphere of radius 0.7,
    # 1 % radial noise): 10 Taubin iterations cut the radial std 2.51x and move the mean radius by +0.034 %; Laplacian (mu = 0) shrinks it
    # by 0.81 %
    (X, Y, Z), sp = lattice((48, 48, 48), -1.0, 1.0)
    v, f, _ = R.marching_cubes((0.7 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))
    v = (v * (1 + 0.01 * np.random.default_rng(5).standard_normal(len(v))).astype(np.float32)[:, None]).astype(np.float32)
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    vt, _ = S.smooth(v, f, 10, 0.5, -0.53)
    vl, _ = S.smooth(v, f, 10, 0.5, 0.0)
    rt, rl = (np.linalg.norm(x.astype(np.float64), axis=1) for x in (vt, vl))
    assert r.std() / rt.std() >= 2.0 and abs(rt.mean() / r.mean() - 1) < 1e-3
    assert rl.mean() / r.mean() - 1 < -5e-3
