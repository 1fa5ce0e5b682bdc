"""GPU: mesh.voxel_remesh — marching cubes over the signed distance of a mesh (csrc/mesh_bvh.hip, k_bvh_signed, through
mesh.sparse_volume and mesh.marching_cubes_sparse) — and extract_mesh(remesh=): closed, manifold output from closed, holed and overlapping
input; vertices within a lattice step of the input surface (a marching-cubes vertex sits on a lattice edge that the zero set crosses);
offsets; the probe=1 result equal to dense marching cubes of the same field, bit for bit; an inward-wound mesh comes out empty; the
renderer's option end to end."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import winding_testlib as L  # noqa: E402
from holes_testlib import holed_sphere  # noqa: E402
from mesh_testlib import AABB, cuda, dtype_guard, gaussian_model, host  # noqa: E402,F401
from ray_testlib import icosphere  # noqa: E402

INFO_KEYS = {'shape', 'origin', 'spacing', 'bricks', 'evaluations', 'rounds', 'offset', 'beta'}


def inradius(v, f):
    """the distance from the origin to the nearest face plane of a convex mesh around it"""
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    return float(np.abs((a * n).sum(1) / np.linalg.norm(n, axis=1)).min())


def test_sphere_is_watertight_and_close():
    from customnerf_amd import mesh
    v, f = icosphere(3)
    gv, gf = cuda(v), cuda(f)
    ov, of, on, info = mesh.voxel_remesh(gv, gf, resolution=48)
    assert set(info) == INFO_KEYS and info['offset'] == 0.0 and info['beta'] == 2.0 and info['bricks'] > 0 and info['rounds'] >= 1
    h = info['spacing'][0]
    side = float((v.max(0) - v.min(0)).max())
    assert info['spacing'] == (h, h, h) and abs(h - side / 47) < 1e-6 and max(info['shape']) == 52       # 48 + 2 pad steps per side
    assert np.abs(np.array(info['origin']) - (v.min(0) - 2 * h)).max() < 1e-6
    assert info['evaluations'] >= 512 * info['bricks']                             # the probe lattice and 8^3 points per brick
    t = mesh.topology(ov, of)
    assert t['watertight'] and t['components'] == 1 and t['euler'] == 2 and of.shape[0] > 5000
    assert ov.dtype == torch.float32 and of.dtype == torch.int32 and on.shape == ov.shape
    d = mesh.closest_point(mesh.build_bvh(gv, gf), ov)['dist2'].sqrt()
    print(f"sphere: {of.shape[0]} faces, max distance to the input {float(d.max()) / h:.3f} steps")
    assert float(d.max()) <= h * (1 + 1e-5)
    # wound outwards, like its input: the normals point away from the centre and the winding number inside is 1
    assert float((on * ov).sum(1).min()) > 0
    assert float(mesh.winding_number(mesh.build_bvh(ov, of), torch.zeros(1, 3, device="cuda"))[0]) > 0.99


def test_holes_are_capped():
    from customnerf_amd import mesh
    v, f, _ = holed_sphere()
    before = mesh.topology(cuda(v), cuda(f))
    assert before['boundary_loops'] == 3 and not before['watertight']
    ov, of, _, info = mesh.voxel_remesh(cuda(v), cuda(f), resolution=48)
    t = mesh.topology(ov, of)
    assert t['boundary_loops'] == 0 and t['boundary_edges'] == 0 and t['watertight'] and t['components'] == 1 and t['euler'] == 2


def test_overlapping_spheres_become_one_shell():
    from customnerf_amd import mesh
    v, f = L.two_spheres(2)
    ov, of, _, info = mesh.voxel_remesh(cuda(v), cuda(f), resolution=48)
    h = info['spacing'][0]
    t = mesh.topology(ov, of)
    assert t['watertight'] and t['components'] == 1 and t['euler'] == 2
    x = host(ov).astype(np.float64)
    depth = np.stack([1.0 - np.linalg.norm(x - np.array([s, 0.0, 0.0]), axis=1) for s in (-0.4, 0.4)], 1)
    print(f"two spheres: deepest output vertex {depth.max() / h:.3f} steps inside an analytic sphere")
    assert depth.max() <= h                                                        # the faces inside the union are gone
    assert depth.max(1).min() >= -h                                                # and every vertex is near one of the two


@pytest.mark.parametrize("steps", [3, -3])
def test_offset(steps):
    from customnerf_amd import mesh
    v, f = icosphere(3)
    r_in, r = inradius(v, f), float(np.linalg.norm(v.astype(np.float64), axis=1).max())
    h = 2.0 / 31
    delta = steps * h
    ov, of, _, info = mesh.voxel_remesh(cuda(v), cuda(f), voxel=h, offset=delta)
    assert info['offset'] == delta and np.abs(np.array(info['origin']) - (v.min(0) - 5 * h)).max() < 1e-6    # |offset| / h + pad steps
    rad = np.linalg.norm(host(ov).astype(np.float64), axis=1)
    print(f"offset {steps:+d} steps: radii in [{rad.min():.4f}, {rad.max():.4f}], allowed [{r_in + delta - h:.4f}, {r + delta + h:.4f}]")
    assert rad.min() >= r_in + delta - h and rad.max() <= r + delta + h
    t = mesh.topology(ov, of)
    assert t['watertight'] and t['components'] == 1 and t['euler'] == 2


def _canonical(faces):
    """triangles as rows starting at their smallest index, sorted: the same set whatever the order they were emitted in"""
    k = faces.argmin(1)
    rolled = np.stack([np.roll(row, -int(s)) for row, s in zip(faces, k)]) if len(faces) else faces
    return rolled[np.lexsort(rolled.T[::-1])]


def test_probe_1_equals_dense_marching_cubes():
    from customnerf_amd import mesh
    v, f = L.FIXTURES["torus"][:2]
    gv, gf = cuda(v), cuda(f)
    ov, of, on, info = mesh.voxel_remesh(gv, gf, resolution=32, probe=1)
    shape, org, sp = info['shape'], info['origin'], info['spacing']
    assert max(shape) == 36
    ijk = torch.stack(torch.meshgrid(*[torch.arange(n, device="cuda") for n in shape], indexing="ij"), -1).reshape(-1, 3)
    pts = (torch.tensor(org, dtype=torch.float32, device="cuda") + ijk.float() * torch.tensor(sp, dtype=torch.float32, device="cuda")).contiguous()
    vol = (-mesh.signed_distance(mesh.build_bvh(gv, gf), pts)['signed']).reshape(shape)
    dv, df, dn = mesh.marching_cubes(vol, 0.0, spacing=sp, origin=org)
    sv = mesh.sparse_volume_from_dense(vol, 0.0, spacing=sp, origin=org)
    assert sv.n_bricks == info['bricks']
    kv, kf, kn, keys = mesh.marching_cubes_sparse(sv, 0.0, want_keys=True)
    assert torch.equal(kv, ov) and torch.equal(kf, of) and torch.equal(kn, on)     # the same bricks, the same order
    perm = torch.argsort(keys)
    assert torch.equal(ov[perm], dv) and torch.equal(on[perm], dn) and dv.shape[0] > 1000
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(len(perm), device="cuda")
    np.testing.assert_array_equal(_canonical(host(inv[of.long()])), _canonical(host(df.long())))


def test_inward_wound_sphere_comes_out_empty():
    from customnerf_amd import mesh
    v, f = icosphere(2)
    ov, of, on, info = mesh.voxel_remesh(cuda(v), cuda(f[:, ::-1].copy()), resolution=32)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and on.shape == (0, 3) and info['bricks'] == 0 and set(info) == INFO_KEYS
    # and a mesh without faces
    ov, of, on, info = mesh.voxel_remesh(cuda(v), torch.zeros(0, 3, dtype=torch.int32, device="cuda"), resolution=32)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and set(info) == INFO_KEYS


def test_extract_mesh_remesh(dtype_guard, tmp_path):
    model = gaussian_model(dtype_guard, False)
    kw = dict(resolution=32, threshold=10.0, aabb=AABB)
    plain = model.extract_mesh(**kw)
    same = model.extract_mesh(remesh=None, **kw)
    assert list(plain) == list(same) and 'remesh' not in plain
    for k in plain:
        assert torch.equal(plain[k], same[k]) if torch.is_tensor(plain[k]) else plain[k] == same[k], k
    m = model.extract_mesh(remesh=40, topology=True, deviation=True, **kw)
    assert set(m['remesh']) == INFO_KEYS and max(m['remesh']['shape']) == 44 and m['remesh']['beta'] == 2.0
    assert m['topology']['watertight'] and m['topology']['components'] == 1 and m['topology']['euler'] == 2
    assert m['deviation'] is not None and 0 < m['deviation']['hausdorff'] < 2 * m['remesh']['spacing'][0]
    assert model.extract_mesh(deviation=True, **kw)['deviation'] is None
    long = model.extract_mesh(remesh=dict(resolution=40, offset=0.0, beta=2.0, probe=2), **kw)
    assert torch.equal(long['verts'], m['verts']) and torch.equal(long['faces'], m['faces'])
    for bad in (True, 2.5, dict(), dict(resolution=40, voxel=0.1), dict(resolution=40, pad=3)):
        with pytest.raises(ValueError, match="remesh"):
            model.extract_mesh(remesh=bad, **kw)
    p = str(tmp_path / "x.glb")
    w = model.save_mesh(p, remesh=40, target_faces=m['faces'].shape[0] // 4, texture=256, **kw)
    assert os.path.getsize(p) > 256 * 256 // 8 and 'remesh' in w and w['texture'].shape == (256, 256, 3)
    assert w['faces'].shape[0] in (m['faces'].shape[0] // 4, m['faces'].shape[0] // 4 - 1)
