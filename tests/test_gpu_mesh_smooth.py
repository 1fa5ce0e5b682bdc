"""GPU: Taubin smoothing and area-weighted vertex normals (csrc/mesh_smooth.hip) against their NumPy restatement
(tests/smooth_restatement.py) — positions and normals bit for bit — their invariants and smoothing behaviour, and end to end through
NeRFRenderer.extract_mesh / save_mesh."""
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
import smooth_restatement as S  # noqa: E402
from mesh_testlib import AABB, cuda, decimate_meshes, dtype_guard, gaussian_model, host, lattice  # noqa: E402,F401

DECIMATE_MESHES = decimate_meshes()

PARAMS = [(1, 0.5, -0.53, True), (10, 0.5, -0.53, True), (7, 0.33, 0.0, False), (4, 1.0, -1.0, True), (3, 0.6307, -0.6732, False)]


def simplified_mesh():
    """clustering output (need not be manifold) of the jittered sphere, with its normals"""
    from customnerf_amd import mesh
    _, v, f, n = DECIMATE_MESHES[0]
    vo, fo, no = mesh.simplify(cuda(v), cuda(f), 0.12, normals=cuda(n))
    return "simplified", host(vo), host(fo), host(no)


@pytest.mark.parametrize("idx", list(range(len(DECIMATE_MESHES) + 1)), ids=[m[0] for m in DECIMATE_MESHES] + ["simplified"])
def test_smooth_matches_restatement(idx):
    from customnerf_amd import mesh
    name, v, f, n = DECIMATE_MESHES[idx] if idx < len(DECIMATE_MESHES) else simplified_mesh()
    L = S.lists(f, len(v))
    assert L["flags"] == 0 and len(f) > 100
    for it, lam, mu, pin in PARAMS:
        vr, nr = S.smooth(v, f, it, lam, mu, pin, normals=n)
        vo, no = mesh.smooth(cuda(v), cuda(f), it, lam, mu, normals=cuda(n), pin_boundary=pin)
        assert torch.equal(vo, cuda(vr)), (name, it, lam, mu, pin)                            # bit for bit
        assert torch.equal(no, cuda(nr)), (name, it, lam, mu, pin)
        if pin:
            fixed = (L["count"] == 0) | L["boundary"]
            np.testing.assert_array_equal(host(vo)[fixed].view(np.uint32), v[fixed].view(np.uint32))
        again = mesh.smooth(cuda(v), cuda(f), it, lam, mu, normals=cuda(n), pin_boundary=pin)
        assert torch.equal(again[0], vo) and torch.equal(again[1], no)                          # deterministic
    assert torch.equal(mesh.vertex_normals(cuda(v), cuda(f), cuda(n)), cuda(S.vertex_normals(v, f, n)))
    v0, n0 = mesh.smooth(cuda(v), cuda(f), 0, normals=cuda(n))
    assert torch.equal(v0, cuda(v)) and torch.equal(n0, cuda(S.vertex_normals(v, f, n)))


def test_cut_sphere_keeps_its_cut():
    from customnerf_amd import mesh
    name, v, f, n = [m for m in DECIMATE_MESHES if m[0] == "cut_sphere"][0]
    extra = np.concatenate([v, np.full((4, 3), 0.25, np.float32)])                             # unreferenced vertices
    b = np.concatenate([v[:, 2] == -1.0, np.zeros(4, bool)])
    assert b.sum() > 20
    vo, no = mesh.smooth(cuda(extra), cuda(f), 10)
    vo = host(vo)
    np.testing.assert_array_equal(vo[b].view(np.uint32), extra[b].view(np.uint32))
    np.testing.assert_array_equal(vo[len(v):].view(np.uint32), extra[len(v):].view(np.uint32))
    assert (host(no)[len(v):] == 0).all()
    assert (vo[:len(v)][~b[:len(v)]] != v[~b[:len(v)]]).any(axis=1).mean() > 0.9


def noisy_sphere():
    (X, Y, Z), sp = lattice((48, 48, 48), -1.0, 1.0)
    v, f, _ = R.marching_cubes((0.7 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))
    v = (v * (1 + 0.01 * np.random.default_rng(5).standard_normal(len(v))).astype(np.float32)[:, None]).astype(np.float32)
    return v, f


def test_taubin_removes_noise_without_shrinking():
    # thresholds from the restatement on the CPU (tests/test_mesh_smooth_host.py, the same mesh): 10 Taubin iterations cut the radial
    # std 2.51x and move the mean radius by +0.034 %; Laplacian smoothing (mu = 0) shrinks it by 0.81 %
    from customnerf_amd import mesh
    v, f = noisy_sphere()
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    vt, nt = mesh.smooth(cuda(v), cuda(f), 10, 0.5, -0.53)
    vl, _ = mesh.smooth(cuda(v), cuda(f), 10, 0.5, 0.0)
    rt, rl = (np.linalg.norm(host(x).astype(np.float64), axis=1) for x in (vt, vl))
    assert r.std() / rt.std() >= 2.0, (r.std(), rt.std())
    assert abs(rt.mean() / r.mean() - 1) < 1e-3, rt.mean() / r.mean() - 1
    assert rl.mean() / r.mean() - 1 < -5e-3, rl.mean() / r.mean() - 1
    assert torch.equal(vt, cuda(S.smooth(v, f, 10, 0.5, -0.53)[0]))
    vt = host(vt)
    assert ((host(nt) * vt).sum(1) / np.linalg.norm(vt, axis=1) > 0.9).all()


def test_normals_of_a_sphere_are_radial():
    from customnerf_amd import mesh
    (X, Y, Z), sp = lattice((128, 128, 128), -1.0, 1.0)
    v, f, nrm = mesh.marching_cubes(cuda((0.7 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)), 0.0, spacing=sp,
                                    origin=(-1.0, -1.0, -1.0))
    radial = torch.nn.functional.normalize(v.double(), dim=1)
    for n in (mesh.vertex_normals(v, f), mesh.smooth(v, f, 10, normals=nrm)[1]):
        assert n.shape == v.shape and bool(torch.isfinite(n).all())
        assert float((n.double() * radial).sum(1).min()) > 0.99
    vs, ns = mesh.smooth(v, f, 10, normals=nrm)
    assert float((ns.double() * torch.nn.functional.normalize(vs.double(), dim=1)).sum(1).min()) > 0.99


def test_errors_and_edge_cases():
    from customnerf_amd import mesh
    v = cuda(np.random.default_rng(0).random((6, 3), dtype=np.float32))
    f = cuda(np.array([[0, 1, 2], [2, 1, 3]], np.int32))
    for bad in ([[0, 1, 6]], [[0, -1, 2]], [[5, 4, 3], [2, 1, 70000]]):
        with pytest.raises(ValueError):
            mesh.smooth(v, cuda(np.array(bad, np.int32)))
        with pytest.raises(ValueError):
            mesh.vertex_normals(v, cuda(np.array(bad, np.int32)))
    for kw in (dict(iterations=-1), dict(lamb=0.0), dict(lamb=1.5), dict(mu=0.1), dict(mu=-1.5), dict(lamb=float("nan")),
               dict(mu=float("-inf"))):
        with pytest.raises(ValueError):
            mesh.smooth(v, f, **kw)
    with pytest.raises(RuntimeError):                                                           # no CPU path
        mesh.smooth(v.cpu(), f.cpu())
    e0, e1 = mesh.smooth(cuda(np.zeros((0, 3), np.float32)), cuda(np.zeros((0, 3), np.int32)))
    assert e0.shape == (0, 3) and e1.shape == (0, 3)
    n_in = cuda(np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (6, 1)))
    vo, no = mesh.smooth(v, cuda(np.zeros((0, 3), np.int32)), 5, normals=n_in)                  # F = 0: nothing moves
    assert torch.equal(vo, v) and torch.equal(no, n_in)
    assert torch.equal(mesh.vertex_normals(v, cuda(np.zeros((0, 3), np.int32))), torch.zeros_like(v))


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_extract_mesh_smooth(dtype_guard, fp16):
    from customnerf_amd import mesh
    model = gaussian_model(dtype_guard, fp16)
    Rn = 96
    plain = model.extract_mesh(resolution=Rn, threshold=10.0, aabb=AABB)
    F = plain['faces'].shape[0]
    target = F // 4
    m = model.extract_mesh(resolution=Rn, threshold=10.0, aabb=AABB, smooth=6, keep_largest=True, target_faces=target)
    v1, f1, n1, _ = mesh.remove_small_components(plain['verts'], plain['faces'], plain['normals'], largest=True)
    v2, n2 = mesh.smooth(v1, f1, 6, normals=n1)
    v3, f3, n3, _ = mesh.decimate(v2, f1, target, normals=n2)
    assert torch.equal(v3, m['verts']) and torch.equal(f3, m['faces']) and torch.equal(n3, m['normals'])
    assert m['faces'].shape[0] in (target - 1, target)
    s = model.extract_mesh(resolution=Rn, threshold=10.0, aabb=AABB, smooth=3, smooth_lambda=0.4, smooth_mu=0.0)
    v4, n4 = mesh.smooth(plain['verts'], plain['faces'], 3, 0.4, 0.0, normals=plain['normals'])
    assert torch.equal(s['verts'], v4) and torch.equal(s['normals'], n4) and torch.equal(s['faces'], plain['faces'])
    assert not torch.equal(v4, plain['verts'])
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=16, aabb=AABB, smooth=-1)
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=16, threshold=10.0, aabb=AABB, smooth=1, smooth_lambda=2.0)


def test_save_mesh_smoothed(dtype_guard, tmp_path):
    from customnerf_amd import mesh
    model = gaussian_model(dtype_guard, False)
    p = str(tmp_path / "blob_smooth.ply")
    m = model.save_mesh(p, resolution=96, threshold=10.0, aabb=AABB, smooth=5, color=True)
    plain = model.extract_mesh(resolution=96, threshold=10.0, aabb=AABB)
    v2, n2 = mesh.smooth(plain['verts'], plain['faces'], 5, normals=plain['normals'])
    back = R.read_ply(p)
    assert np.array_equal(back["verts"], host(v2)) and np.array_equal(back["normals"], host(n2))
    assert np.array_equal(back["faces"], host(plain['faces']))
    assert torch.equal(m['verts'], v2) and torch.equal(m['normals'], n2)
    with torch.no_grad():
        rgb = model(m['verts'], -m['normals'])[1][:, :3].float().clamp(0, 1)                   # sampled along the recomputed normals
    np.testing.assert_array_equal(back["colors"], (rgb * 255).round().to(torch.uint8).cpu().numpy())
