"""GPU: mesh cleanup (csrc/mesh_clean.hip) against its NumPy restatement (tests/mesh_clean_restatement.py) — component removal exact,
clustering with the same faces and positions to 1e-4 cell — and end to end through NeRFRenderer.extract_mesh / save_mesh."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mc_restatement as R  # noqa: E402
import mesh_clean_restatement as MC  # noqa: E402
from mesh_testlib import AABB, R_SPHERE, cuda, dtype_guard, gaussian_model, host, lattice, speckled_sphere  # noqa: E402,F401


def mc_meshes():
    rng = np.random.default_rng(17)
    _, vol, sp, org = speckled_sphere()
    yield ("speckled_sphere",) + R.marching_cubes(vol, 0.0, sp, org)
    (X, Y, Z), sp = lattice((64, 48, 40), -1.0, 1.0)
    t1 = 0.15 - np.sqrt((np.sqrt((X + 0.45) ** 2 + Y ** 2) - 0.35) ** 2 + Z ** 2)
    t2 = 0.1 - np.sqrt((np.sqrt((X - 0.5) ** 2 + Z ** 2) - 0.3) ** 2 + Y ** 2)
    yield ("two_tori",) + R.marching_cubes(np.maximum(t1, t2).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))
    yield ("noise",) + R.marching_cubes(rng.random((28, 28, 28), dtype=np.float32), 0.55, (0.5, 0.25, 1.0), (3.0, -2.0, 0.5))


def hand_meshes():
    v = np.arange(3 * 15, dtype=np.float32).reshape(-1, 3) * np.float32(0.37)
    f = np.array([[0, 1, 2], [3, 4, 5], [5, 6, 7], [8, 9, 10], [10, 9, 11]], dtype=np.int32)
    yield "disjoint_unreferenced", v, f, None                                        # vertices 12..14 unreferenced
    f2 = np.array([[0, 1, 2], [0, 1, 2], [2, 1, 0], [3, 3, 4], [4, 5, 6], [6, 5, 4], [1, 2, 0]], dtype=np.int32)
    n2 = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (len(v), 1))
    yield "duplicate_degenerate", v, f2, n2
    yield "empty", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None
    yield "no_faces", v[:5], np.zeros((0, 3), np.int32), None


MESHES = [(name, v, f, n) for name, v, f, n in mc_meshes()] + list(hand_meshes())
IDS = [m[0] for m in MESHES]


@pytest.mark.parametrize("name,v,f,n", MESHES, ids=IDS)
def test_components_match_restatement(name, v, f, n):
    from customnerf_amd import mesh
    V = len(v)
    for min_faces, largest in ((0, False), (1, False), (3, False), (40, False), (0, True), (10, True), (10 ** 9, False)):
        ref = MC.components(v, f, n, min_faces=min_faces, largest=largest)
        out = mesh.remove_small_components(cuda(v), cuda(f), cuda(n), min_faces=min_faces, largest=largest)
        again = mesh.remove_small_components(cuda(v), cuda(f), cuda(n), min_faces=min_faces, largest=largest)
        vo, fo, no, old = (host(t) for t in out)
        np.testing.assert_array_equal(fo, ref[1])
        np.testing.assert_array_equal(old, ref[3])
        np.testing.assert_array_equal(vo.view(np.uint32), ref[0].view(np.uint32))                 # copies: bit-equal
        if n is not None:
            np.testing.assert_array_equal(no.view(np.uint32), ref[2].view(np.uint32))
        for a, b in zip(out, again):                                                             # deterministic
            if a is not None:
                assert torch.equal(a, b)
        if min_faces == 0 and not largest:                                                       # identity
            assert np.array_equal(vo, v) and np.array_equal(fo, f) and np.array_equal(old, np.arange(V))


@pytest.mark.parametrize("name,v,f,n", MESHES, ids=IDS)
def test_cluster_matches_restatement(name, v, f, n):
    from customnerf_amd import mesh
    if name in ("speckled_sphere", "two_tori"):
        cells = (0.09, (0.07, 0.11, 0.05))
    elif name == "noise":
        cells = (1.1, 2.0)
    else:
        cells = (0.5, 1.9)
    for cell in cells:
        o, c, g = MC.default_grid(v, cell) if len(v) else (np.zeros(3, np.float32), np.full(3, cell, np.float32), (1, 1, 1))
        vr, fr, nr, flagged = MC.cluster(v, f, o, c, g, normals=n)
        out = mesh.simplify(cuda(v), cuda(f), cell, normals=cuda(n))
        again = mesh.simplify(cuda(v), cuda(f), cell, normals=cuda(n))
        vo, fo, no = (host(t) for t in out)
        np.testing.assert_array_equal(fo, fr)
        assert vo.shape == vr.shape
        err = (np.abs(vo.astype(np.float64) - vr) / c).max(axis=1) if len(vo) else np.zeros(0)
        assert (err[~flagged] <= 1e-4).all(), f"{name} cell {cell}: max |dx| / cell = {err[~flagged].max():.3g} away from the cutoff"
        # The sums are restated exactly, so even near the cutoff only a last-bit disagreement of the two eigen-solvers can differ.
        assert err.size == 0 or (err <= 1e-4).mean() >= 0.99
        if n is not None:
            np.testing.assert_allclose(no, nr, rtol=0, atol=1e-6)
        for a, b in zip(out, again):                                                             # deterministic
            if a is not None:
                assert torch.equal(a, b)
        if len(vo):
            lo, hi = o.astype(np.float64), o + c.astype(np.float64) * np.array(g)
            assert (vo >= lo - 1e-6).all() and (vo <= hi + 1e-6).all()


def test_bad_face_index_raises():
    from customnerf_amd import mesh
    v = cuda(np.random.default_rng(0).random((6, 3), dtype=np.float32))
    for bad in ([[0, 1, 6]], [[0, -1, 2]], [[5, 4, 3], [2, 1, 70000]]):
        f = cuda(np.array(bad, dtype=np.int32))
        with pytest.raises(ValueError):
            mesh.remove_small_components(v, f)
        with pytest.raises(ValueError):
            mesh.simplify(v, f, 0.25)


def test_largest_of_speckled_sphere_is_the_sphere():
    from customnerf_amd import mesh
    sphere, vol, sp, org = speckled_sphere()
    vs, fs, ns = R.marching_cubes(sphere, 0.0, sp, org)
    v, f, n = R.marching_cubes(vol, 0.0, sp, org)
    assert len(f) > len(fs)                                                                      # the speckle is there
    vo, fo, no, old = (host(t) for t in mesh.remove_small_components(cuda(v), cuda(f), cuda(n), largest=True))
    np.testing.assert_array_equal(vo.view(np.uint32), vs.view(np.uint32))
    np.testing.assert_array_equal(fo, fs)
    np.testing.assert_array_equal(no.view(np.uint32), ns.view(np.uint32))
    assert R.check_closed_oriented(vo, fo) == 0 and R.euler_characteristic(vo, fo) == 2
    # min_faces between the largest blob and the sphere gives the same mesh
    vo2, fo2, _, _ = (host(t) for t in mesh.remove_small_components(cuda(v), cuda(f), None, min_faces=len(fs) // 2))
    assert np.array_equal(fo2, fs) and np.array_equal(vo2, vs)


# ------------------------------------------------------------------------------------------------ end to end through NeRFNetwork
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_extract_mesh_cleanup(dtype_guard, fp16):
    model = gaussian_model(dtype_guard, fp16)
    Rn = 128
    plain = model.extract_mesh(resolution=Rn, threshold=10.0, aabb=AABB)
    big = model.extract_mesh(resolution=Rn, threshold=10.0, aabb=AABB, keep_largest=True, min_component_faces=100)
    for k in ('verts', 'faces', 'normals'):
        assert torch.equal(plain[k], big[k]), k                                 # one component: bit-identical
    F = plain['faces'].shape[0]
    none = model.extract_mesh(resolution=Rn, threshold=10.0, aabb=AABB, min_component_faces=F + 1)
    assert none['verts'].shape == (0, 3) and none['faces'].shape == (0, 3) and none['normals'].shape == (0, 3)
    s = model.extract_mesh(resolution=Rn, threshold=10.0, aabb=AABB, simplify=4)
    v, f = s['verts'].cpu().numpy(), s['faces'].cpu().numpy()
    # Measured on the MI355X: 37,724 -> 2,232 faces (16.9x) and 18,864 -> 1,118 vertices in fp32 and fp16, against the 4x used here;
    # max |r - R| = 7.08e-4 against the cluster diagonal 5.46e-2.
    assert len(f) * 4 <= F and len(f) > 100
    cell = 4 * 1.0 / (Rn - 1)
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    assert np.abs(r - R_SPHERE).max() <= math.sqrt(3) * cell                   # within one cluster diagonal
    n = s['normals'].cpu().numpy()
    assert ((n * v).sum(1) > 0).all()                                          # outward
    fn = R.face_normals(v, f)
    assert ((fn * v[f].mean(1)).sum(1) > 0).mean() > 0.99                      # winding kept
    # the cleanup is the library's: the same as mesh.* on the plain mesh
    from customnerf_amd import mesh
    lo = np.array(AABB[:3], np.float32)
    step = (np.array(AABB[3:], np.float32) - lo) / np.float32(Rn - 1)
    g = (-(-(Rn - 1) // 4),) * 3
    v2, f2, n2 = mesh.simplify(plain['verts'], plain['faces'], (step * 4).tolist(), normals=plain['normals'], origin=lo.tolist(), grid=g)
    assert torch.equal(v2, s['verts']) and torch.equal(f2, s['faces']) and torch.equal(n2, s['normals'])


def test_save_mesh_simplified_with_colors(dtype_guard, tmp_path):
    model = gaussian_model(dtype_guard, False)
    p = str(tmp_path / "blob_s4.ply")
    m = model.save_mesh(p, resolution=96, threshold=10.0, aabb=AABB, simplify=4, keep_largest=True, color=True)
    back = R.read_ply(p)
    assert len(back["verts"]) == m['verts'].shape[0] and len(back["faces"]) == m['faces'].shape[0] and len(back["faces"]) > 50
    assert np.array_equal(back["verts"], m['verts'].cpu().numpy()) and np.array_equal(back["faces"], m['faces'].cpu().numpy())
    c = back["colors"]
    assert c.dtype == np.uint8 and c.shape == (len(back["verts"]), 3)
    with torch.no_grad():
        rgb = model(m['verts'], -m['normals'])[1][:, :3].float().clamp(0, 1)   # sampled at the final vertices
    np.testing.assert_array_equal(c, (rgb * 255).round().to(torch.uint8).cpu().numpy())
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=16, aabb=AABB, simplify=1)
