"""GPU: marching cubes (csrc/mesh.hip) against its NumPy restatement (tests/mc_restatement.py) — same faces, bit-equal vertices — and mesh
export end to end through NeRFNetwork (NeRFRenderer.extract_mesh / save_mesh)."""
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
from mesh_testlib import R_SPHERE, dtype_guard, gaussian_model, lattice  # noqa: E402,F401


def volumes():
    rng = np.random.default_rng(7)
    (X, Y, Z), sp = lattice((40, 40, 40), -1.0, 1.0)
    yield "sphere", (1 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), 0.45, sp, (-1.0, -1.0, -1.0)
    (X, Y, Z), sp = lattice((48, 44, 36), -1.0, 1.0)
    q = np.sqrt(X ** 2 + Y ** 2) - 0.6
    yield "torus", (0.25 - np.sqrt(q ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0)
    yield "noise", rng.random((32, 32, 32), dtype=np.float32), 0.5, (0.5, 0.25, 2.0), (3.0, -2.0, 0.5)
    yield "constant", np.full((16, 16, 16), 3.0, dtype=np.float32), 3.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    v = rng.standard_normal((33, 17, 9)).astype(np.float32)
    v[rng.random(v.shape) < 0.02] = np.nan                                      # NaN corners are outside (and give t = 0.5)
    yield "non_cubic", v, 0.1, (0.1, 0.2, 0.3), (-1.0, 0.0, 1.0)
    (X, Y, Z), sp = lattice((160, 170, 180), -1.0, 1.0)                         # 19 k workgroups: several tiles of the one-workgroup scan
    yield "large", (np.sin(5 * X) * np.cos(4 * Y) + np.sin(3 * Z)).astype(np.float32), 0.2, sp, (-1.0, -1.0, -1.0)


CASES = list(volumes())


@pytest.mark.parametrize("name,vol,level,sp,org", CASES, ids=[c[0] for c in CASES])
def test_marching_cubes_matches_restatement(name, vol, level, sp, org):
    from customnerf_amd import mesh
    v_ref, f_ref, n_ref = R.marching_cubes(vol, level, sp, org)
    g = torch.from_numpy(vol).cuda()
    v, f, n = mesh.marching_cubes(g, level, spacing=sp, origin=org)
    v2, f2, n2 = mesh.marching_cubes(g, level, spacing=sp, origin=org)
    torch.cuda.synchronize()
    v, f, n = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    assert v.shape == v_ref.shape and f.shape == f_ref.shape
    np.testing.assert_array_equal(f, f_ref)
    np.testing.assert_array_equal(v.view(np.uint32), v_ref.view(np.uint32))     # bit-equal positions
    np.testing.assert_allclose(n, n_ref, rtol=0, atol=2e-6)
    # deterministic: a second run is bit-identical
    np.testing.assert_array_equal(v2.cpu().numpy().view(np.uint32), v.view(np.uint32))
    np.testing.assert_array_equal(n2.cpu().numpy().view(np.uint32), n.view(np.uint32))
    np.testing.assert_array_equal(f2.cpu().numpy(), f)
    if name == "constant":
        assert len(v) == 0 and len(f) == 0
    if name in ("sphere", "torus"):
        assert R.check_closed_oriented(v, f) == 0
        assert R.euler_characteristic(v, f) == (2 if name == "sphere" else 0)


def test_emit_respects_capacity():
    """counts above max_verts / max_faces: the first max_* entries are the full run's, nothing past them is written"""
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib, check, ptr, stream
    import ctypes as C
    vol = np.random.default_rng(11).random((24, 20, 28), dtype=np.float32)
    v_ref, f_ref, n_ref = R.marching_cubes(vol, 0.5)
    g = torch.from_numpy(vol).cuda()
    nx, ny, nz = vol.shape
    nbytes = mesh.workspace_bytes(vol.shape)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    check(lib.cnerf_marching_cubes_count(ptr(g), nx, ny, nz, 0.5, ptr(ws), nbytes, ptr(counts), stream()), "count")
    V, F = (int(c) for c in counts.cpu())
    assert (V, F) == (len(v_ref), len(f_ref))
    mv, mf = V // 3, F // 2
    verts = torch.full((V + 64, 3), -7.0, device="cuda")
    nrm = torch.full((V + 64, 3), -7.0, device="cuda")
    faces = torch.full((F + 64, 3), -7, dtype=torch.int32, device="cuda")
    org, sp = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    check(lib.cnerf_marching_cubes_emit(ptr(g), nx, ny, nz, 0.5, org, sp, ptr(ws), nbytes, ptr(verts), ptr(nrm), ptr(faces), mv, mf, stream()),
          "emit")
    verts, nrm, faces = verts.cpu().numpy(), nrm.cpu().numpy(), faces.cpu().numpy()
    np.testing.assert_array_equal(verts[:mv], v_ref[:mv])
    np.testing.assert_allclose(nrm[:mv], n_ref[:mv], rtol=0, atol=2e-6)
    np.testing.assert_array_equal(faces[:mf], f_ref[:mf])
    assert (verts[mv:] == -7.0).all() and (nrm[mv:] == -7.0).all() and (faces[mf:] == -7).all()


# ------------------------------------------------------------------------------------------------ end to end through NeRFNetwork
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_extract_mesh_gaussian_sphere(dtype_guard, fp16):
    model = gaussian_model(dtype_guard, fp16)
    m = model.extract_mesh(resolution=128, threshold=10.0, aabb=[-0.5, -0.5, -0.5, 0.5, 0.5, 0.5])
    v, f, n = m['verts'].cpu().numpy(), m['faces'].cpu().numpy(), m['normals'].cpu().numpy()
    assert m['volume'].shape == (128, 128, 128) and len(f) > 1000
    assert R.check_closed_oriented(v, f) == 0                                  # watertight, consistently wound
    assert R.euler_characteristic(v, f) == 2
    fn = R.face_normals(v, f)
    assert ((fn * v[f].mean(1)).sum(1) > 0).all()                              # outward faces
    assert ((n * v).sum(1) > 0).all()                                          # outward vertex normals
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    # The fused field evaluates the blob in float32 in both precisions (fp16 only rounds the zeroed density network's output, which is 0).
    # Measured on the MI355X: max |r - R| = 1.217e-4 (fp32) and 1.217e-4 (fp16), against the bound of one voxel (7.87e-3) used here.
    assert np.abs(r - R_SPHERE).max() <= 1.0 / 127


def test_extract_mesh_part_masks_like_run(dtype_guard):
    model = gaussian_model(dtype_guard, False)
    Rn, aabb, d = 24, [-0.6, -0.6, -0.6, 0.6, 0.6, 0.6], (0.0, 0.0, -1.0)
    lin = torch.arange(Rn, device="cuda").float()
    ijk = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(-1, 3)
    lo = torch.tensor(aabb[:3], device="cuda")
    step = ((torch.tensor(aabb[3:]) - torch.tensor(aabb[:3])) / (Rn - 1)).cuda()
    x = (lo + ijk * step).contiguous()
    with torch.no_grad():
        sigma, rgbc, _ = model(x, torch.tensor(d, device="cuda").expand(len(x), 3).contiguous())
    sigma, conf = sigma.reshape(-1, 1).float(), rgbc[:, 3:4].float()
    for soft in (True, False):
        model.opt.soft_mask = soft
        # renderer.py:386-395
        if soft:
            edit_mask = torch.sigmoid((conf - model.opt.conf_thr) * 100)
            fg, bg = sigma.clone() * edit_mask, sigma.clone() * (1 - edit_mask)
        else:
            edit_mask = conf > 0.5
            bg = sigma.clone()
            bg[edit_mask] = 0
            fg = sigma.clone()
            fg[~edit_mask] = 0
        for part, ref in (("fg", fg), ("bg", bg)):
            vol = model.density_volume(Rn, aabb=aabb, part=part, view_dir=d)
            torch.testing.assert_close(vol.reshape(-1), ref.reshape(-1), rtol=0, atol=0)
    model.opt.soft_mask = True
    m = model.extract_mesh(resolution=Rn, threshold=10.0, aabb=aabb, part='fg')
    fg_soft = sigma.clone() * torch.sigmoid((conf - model.opt.conf_thr) * 100)
    torch.testing.assert_close(m['volume'].reshape(-1), fg_soft.reshape(-1), rtol=0, atol=0)
    plain = gaussian_model(dtype_guard, False, train_conf=0)
    with pytest.raises(ValueError):
        plain.extract_mesh(resolution=8, part='fg')


def test_save_mesh_with_colors(dtype_guard, tmp_path):
    model = gaussian_model(dtype_guard, False)
    p = str(tmp_path / "blob.ply")
    m = model.save_mesh(p, resolution=48, threshold=10.0, aabb=[-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], color=True)
    back = R.read_ply(p)
    assert np.array_equal(back["verts"], m['verts'].cpu().numpy())
    assert np.array_equal(back["faces"], m['faces'].cpu().numpy())
    c = back["colors"]
    assert c.dtype == np.uint8 and c.shape == (len(back["verts"]), 3) and len(c) > 100
    with torch.no_grad():
        rgb = model(m['verts'], -m['normals'])[1][:, :3].float().clamp(0, 1)
    np.testing.assert_array_equal(c, (rgb * 255).round().to(torch.uint8).cpu().numpy())
    assert np.isfinite(back["normals"]).all()


def test_convert_sigma_samples_to_ply(tmp_path):
    from customnerf_amd.nerf.renderer import convert_sigma_samples_to_ply
    (X, Y, Z), sp = lattice((30, 30, 30), -1.0, 1.0)
    vol = (10 * (1 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2))).astype(np.float32)
    p = str(tmp_path / "s.ply")
    verts, faces, normals = convert_sigma_samples_to_ply(vol, [-1, -1, -1], sp, p, level=5.0, offset=np.array([0.5, 0, 0]), scale=2.0)
    v_ref, f_ref, _ = R.marching_cubes(vol, 5.0, sp, (0, 0, 0))
    np.testing.assert_array_equal(verts, v_ref)
    np.testing.assert_array_equal(faces, f_ref)
    back = R.read_ply(p)
    np.testing.assert_allclose(back["verts"], (v_ref + np.float32(-1)) / 2.0 - np.array([0.5, 0, 0]), rtol=0, atol=1e-6)
    assert normals.shape == verts.shape
