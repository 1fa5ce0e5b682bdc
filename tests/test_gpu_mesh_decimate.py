"""GPU: quadric edge-collapse decimation (csrc/mesh_decimate.hip) against its NumPy restatement (tests/qem_restatement.py) — faces,
old_index, per-round counts and positions exactly — its properties on larger marching-cubes meshes, and end to end through
NeRFRenderer.extract_mesh / save_mesh."""
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
import qem_restatement as Q  # noqa: E402
from mesh_testlib import AABB, R_SPHERE, cuda, decimate_meshes, dtype_guard, gaussian_model, host, lattice  # noqa: E402,F401

MESHES = decimate_meshes()
IDS = [m[0] for m in MESHES]


@pytest.mark.parametrize("name,v,f,n", MESHES, ids=IDS)
def test_decimate_matches_restatement(name, v, f, n):
    from customnerf_amd import mesh
    F = len(f)
    assert F >= (512 if name == "planar_grid" else 2000)
    for target in (F // 2, F // 5, F // 25):
        vr, fr, nr, oldr, rr = Q.decimate(v, f, target, normals=n)
        rounds = []
        out = mesh.decimate(cuda(v), cuda(f), target, normals=cuda(n), rounds=rounds)
        vo, fo, no, old = (host(t) for t in out)
        assert rounds == [tuple(r) for r in rr], name
        np.testing.assert_array_equal(fo, fr)
        np.testing.assert_array_equal(old, oldr)
        assert torch.equal(out[0], cuda(vr))                                                   # bit for bit
        if n is not None:
            assert torch.equal(out[2], cuda(nr))
        if rounds[-1][2] > 0:
            assert len(fo) in (target - 1, target)
        again = mesh.decimate(cuda(v), cuda(f), target, normals=cuda(n))
        for a, b in zip(out, again):                                                           # deterministic
            if a is not None:
                assert torch.equal(a, b)


def scale_mesh(kind, n=128):
    (X, Y, Z), sp = lattice((n, n, n), -1.0, 1.0)
    if kind == "sphere":
        vol = 0.7 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)
    else:
        vol = 0.2 - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 0.55) ** 2 + Z ** 2)
    from customnerf_amd import mesh
    v, f, nrm = mesh.marching_cubes(cuda(vol.astype(np.float32)), 0.0, spacing=sp, origin=(-1.0, -1.0, -1.0))
    return v, f, nrm, sp[0]


def surface_distance(kind, v):
    v = v.astype(np.float64)
    if kind == "sphere":
        return np.abs(np.linalg.norm(v, axis=1) - 0.7)
    return np.abs(np.sqrt((np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2) - 0.55) ** 2 + v[:, 2] ** 2) - 0.2)


@pytest.mark.parametrize("kind,chi", [("sphere", 2), ("torus", 0)])
def test_properties_at_scale(kind, chi):
    from customnerf_amd import mesh
    v, f, nrm, step = scale_mesh(kind)
    F = f.shape[0]
    target = F // 50
    rounds = []
    vo, fo, no, old = mesh.decimate(v, f, target, normals=nrm, rounds=rounds)
    vh, fh = host(vo), host(fo)
    assert len(fh) in (target - 1, target)
    assert Q.check_manifold(fh) == 0                                                           # closed, oriented, no repeated index
    assert Q.euler(fh) == chi
    assert surface_distance(kind, vh).max() <= step
    assert len(vh) == rounds[-1][0] and sum(r[2] for r in rounds) == (F - len(fh)) // 2
    np.testing.assert_array_equal(host(no), host(nrm)[host(old)])
    if kind == "sphere":
        # against clustering at the face count it reaches
        sv, sf, _ = mesh.simplify(v, f, 4 * step)
        dv, df, _, _ = mesh.decimate(v, f, sf.shape[0])
        rms_c = math.sqrt((surface_distance(kind, host(sv)) ** 2).mean())
        rms_q = math.sqrt((surface_distance(kind, host(dv)) ** 2).mean())
        assert df.shape[0] <= sf.shape[0] and rms_q <= rms_c, (rms_q, rms_c)


def test_edge_cases():
    from customnerf_amd import mesh
    v, f, nrm, _ = scale_mesh("sphere", 16)
    vo, fo, no, old = mesh.decimate(v, f, f.shape[0], normals=nrm)                              # target >= F: unchanged
    assert torch.equal(vo, v) and torch.equal(fo, f) and torch.equal(no, nrm)
    assert torch.equal(old, torch.arange(v.shape[0], device=old.device, dtype=torch.int32))
    e = mesh.decimate(cuda(np.zeros((0, 3), np.float32)), cuda(np.zeros((0, 3), np.int32)), 10)
    assert all(t.shape[0] == 0 for t in (e[0], e[1], e[3]))
    extra = torch.cat([v, torch.zeros(5, 3, device=v.device)])                                  # unreferenced vertices are dropped
    vo, fo, _, old = mesh.decimate(extra, f, 10 ** 9)
    assert torch.equal(vo, v) and torch.equal(fo, f)
    tv = cuda(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32))              # tetrahedron: no valid collapse
    tf = cuda(np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32))
    rounds = []
    vo, fo, _, _ = mesh.decimate(tv, tf, 0, rounds=rounds)
    assert torch.equal(fo, tf) and torch.equal(vo, tv) and rounds == [(4, 4, 0)]


def test_errors():
    from customnerf_amd import mesh
    v = cuda(np.random.default_rng(0).random((6, 3), dtype=np.float32))
    bad = {"index": [[0, 1, 6]], "negative": [[0, -1, 2]], "three_faces": [[0, 1, 2], [1, 0, 3], [0, 1, 4]],
           "same_direction": [[0, 1, 2], [0, 1, 3]], "repeated": [[0, 1, 1], [2, 3, 4]]}
    for name, faces in bad.items():
        with pytest.raises(ValueError):
            mesh.decimate(v, cuda(np.array(faces, np.int32)), 1)
    with pytest.raises(ValueError):
        mesh.decimate(v, cuda(np.array([[0, 1, 2]], np.int32)), -1)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_extract_mesh_target_faces(dtype_guard, fp16):
    from customnerf_amd import mesh
    model = gaussian_model(dtype_guard, fp16)
    Rn = 96
    plain = model.extract_mesh(resolution=Rn, threshold=10.0, aabb=AABB)
    F = plain['faces'].shape[0]
    target = F // 10
    m = model.extract_mesh(resolution=Rn, threshold=10.0, aabb=AABB, keep_largest=True, target_faces=target)
    assert m['faces'].shape[0] in (target - 1, target)
    v2, f2, n2, _ = mesh.decimate(plain['verts'], plain['faces'], target, normals=plain['normals'])
    assert torch.equal(v2, m['verts']) and torch.equal(f2, m['faces']) and torch.equal(n2, m['normals'])
    v = m['verts'].cpu().numpy().astype(np.float64)
    step = 1.0 / (Rn - 1)
    assert np.abs(np.linalg.norm(v, axis=1) - R_SPHERE).max() <= 2 * step
    assert Q.check_manifold(m['faces'].cpu().numpy()) == 0
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=16, aabb=AABB, simplify=2, target_faces=100)
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=16, aabb=AABB, target_faces=-1)


def test_save_mesh_decimated_with_colors(dtype_guard, tmp_path):
    model = gaussian_model(dtype_guard, False)
    p = str(tmp_path / "blob_qem.ply")
    m = model.save_mesh(p, resolution=96, threshold=10.0, aabb=AABB, keep_largest=True, target_faces=1000, color=True)
    back = R.read_ply(p)
    assert len(back["faces"]) == m['faces'].shape[0] and len(back["faces"]) in (999, 1000)
    assert len(back["verts"]) == m['verts'].shape[0]
    assert np.array_equal(back["verts"], m['verts'].cpu().numpy()) and np.array_equal(back["faces"], m['faces'].cpu().numpy())
    c = back["colors"]
    assert c.dtype == np.uint8 and c.shape == (len(back["verts"]), 3)
    with torch.no_grad():
        rgb = model(m['verts'], -m['normals'])[1][:, :3].float().clamp(0, 1)                     # sampled at the final vertices
    np.testing.assert_array_equal(c, (rgb * 255).round().to(torch.uint8).cpu().numpy())
