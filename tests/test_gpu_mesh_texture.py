"""GPU: texture baking (csrc/mesh_texture.hip) against its NumPy restatement (tests/atlas_restatement.py) — UVs and points bit-equal,
directions to 2e-6 — a colour affine in position reproduced by bilinear lookup of the written PNG through the written OBJ's UVs, the store
against the field's own colours, and end to end through NeRFRenderer.save_mesh(..., texture=)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import atlas_restatement as A  # noqa: E402
import mc_restatement as R  # noqa: E402
from mesh_testlib import AABB, cuda, dtype_guard, gaussian_model, lattice  # noqa: E402,F401


def sphere_mesh(n=40, r=0.9):
    (X, Y, Z), sp = lattice((n, n, n), -1.0, 1.0)
    return R.marching_cubes((r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))


def torus_mesh():
    (X, Y, Z), sp = lattice((48, 44, 36), -1.0, 1.0)
    q = np.sqrt(X ** 2 + Y ** 2) - 0.6
    return R.marching_cubes((0.25 - np.sqrt(q ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))


def hand_meshes():
    rng = np.random.default_rng(9)
    v = rng.standard_normal((30, 3)).astype(np.float32)
    f = rng.permutation(30).reshape(10, 3).astype(np.int32)
    yield "soup", v, f, None, 64
    nrm = rng.standard_normal((30, 3)).astype(np.float32)
    nrm[:4] = 0                                                              # zero normals: the interpolated one can vanish
    f2 = np.concatenate([f, [[0, 0, 1], [2, 2, 2], [0, 1, 2]]]).astype(np.int32)   # zero-area faces: no geometric normal either
    yield "soup_normals_degenerate", v, f2, nrm, 37
    yield "one_face", v, f[:1], None, 16


def mc_meshes():
    v, f, n = sphere_mesh()
    yield "sphere", v, f, n, 512
    yield "sphere_s4", v, f, n, 4 * A.layout(len(f), 4096)[0]              # cells of exactly 4 texels
    v, f, n = torus_mesh()
    yield "torus", v, f, n, 1000


MESHES = list(hand_meshes()) + list(mc_meshes())


def atlas_uvs(v, f, Rr, max_faces=None):
    from customnerf_amd._lib import lib, check, ptr, stream
    F = f.shape[0]
    uvs = torch.full((F + 8, 3, 2), -7.0, device="cuda")
    flags = torch.full((1,), 0x55, dtype=torch.int32, device="cuda")
    check(lib.cnerf_mesh_atlas_uvs(ptr(f) if F else None, v.shape[0], F, Rr, ptr(uvs), F if max_faces is None else max_faces, ptr(flags),
                                   stream()), "uvs")
    return uvs, flags


def atlas_points(v, f, n, Rr, flags, t0, t1, max_points=None):
    from customnerf_amd._lib import lib, check, ptr, stream
    N = t1 - t0
    x = torch.full((N + 8, 3), -7.0, device="cuda")
    d = torch.full((N + 8, 3), -7.0, device="cuda")
    check(lib.cnerf_mesh_atlas_points(ptr(v), ptr(n), v.shape[0], ptr(f), f.shape[0], Rr, t0, t1, ptr(flags), ptr(x), ptr(d),
                                      N if max_points is None else max_points, stream()), "points")
    return x, d


@pytest.mark.parametrize("name,v,f,n,Rr", MESHES, ids=[m[0] for m in MESHES])
def test_uvs_and_points_match_restatement(name, v, f, n, Rr):
    F = len(f)
    _, s = A.layout(F, Rr)
    total = (F + 1) // 2 * s * s
    gv, gf, gn = cuda(v), cuda(f), cuda(n)
    runs = []
    for _ in range(2):
        uvs, flags = atlas_uvs(gv, gf, Rr)
        x, d = atlas_points(gv, gf, gn, Rr, flags, 0, total)
        runs.append([t.cpu().numpy() for t in (uvs, flags, x, d)])
    uvs, flags, x, d = runs[0]
    assert flags[0] == 0
    np.testing.assert_array_equal(uvs[:F].view(np.uint32), A.uvs(F, Rr).view(np.uint32))
    assert (uvs[F:] == -7.0).all() and (x[total:] == -7.0).all() and (d[total:] == -7.0).all()
    xr, dr = A.points(v, f, Rr, normals=n)
    np.testing.assert_array_equal(x[:total].view(np.uint32), xr.view(np.uint32))
    np.testing.assert_allclose(d[:total], dr, rtol=0, atol=2e-6)
    np.testing.assert_allclose(np.linalg.norm(d[:total], axis=1), 1.0, atol=1e-6)
    for a, b in zip(runs[0], runs[1]):                                           # a second run is bit-identical
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    # chunks: [t0, t1) pieces give the same rows as the whole range
    t0, t1 = total // 3, total // 3 + max(1, total // 5)
    xc, dc = atlas_points(gv, gf, gn, Rr, cuda(flags), t0, t1)
    np.testing.assert_array_equal(xc[:t1 - t0].cpu().numpy(), x[t0:t1])
    np.testing.assert_array_equal(dc[:t1 - t0].cpu().numpy(), d[t0:t1])


@pytest.mark.parametrize("cell", [6, 4], ids=["s6", "s4"])
def test_affine_colour_bake(tmp_path, cell):
    """colour = 0.5 + 0.4 x baked, written (OBJ + PNG), read back: bilinear lookup at random points of every UV triangle gives the colour
    of the surface point within the uint8 rounding (a wrong owner, a seam bleed, a v-flip or a wrong barycentric all break it)"""
    from customnerf_amd import mesh
    v, f, n = sphere_mesh()
    Rr = cell * A.layout(len(f), 16384)[0]                                     # cells of `cell` texels (s = 4: the tightest insets)
    assert A.layout(len(f), Rr)[1] == cell
    uvs, tex = mesh.bake_texture(cuda(v), cuda(f), Rr, lambda x, d: 0.5 + 0.4 * x, normals=cuda(n), chunk=100_000)
    p = str(tmp_path / "affine.obj")
    mesh.write_obj(p, v, f, uvs=uvs, normals=n, texture=tex)
    o = A.read_obj(p)
    img = A.read_png(str(tmp_path / "affine.png"))
    np.testing.assert_array_equal(img, tex.cpu().numpy())
    assert np.array_equal(o["verts"], v) and np.array_equal(o["f"][..., 0] - 1, f)
    uv = o["uvs"][o["f"][..., 1] - 1].astype(np.float64)                        # [F, 3, 2] through the OBJ's own indices
    np.testing.assert_array_equal(o["uvs"].reshape(-1, 3, 2), A.uvs(len(f), Rr))
    rng = np.random.default_rng(0)
    w = np.concatenate([np.eye(3), [[0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]], rng.dirichlet((1, 1, 1), 10)])   # [K, 3]
    pts_uv = np.einsum("kc,fcd->fkd", w, uv).reshape(-1, 2)
    pts = np.einsum("kc,fcd->fkd", w, v[f].astype(np.float64)).reshape(-1, 3)
    got = A.bilinear(img, pts_uv[:, 0], pts_uv[:, 1]) / 255.0
    err = np.abs(got - (0.5 + 0.4 * pts))
    assert err.max() <= 0.6 / 255, err.max()
    # a v-flipped lookup would not pass: the check has teeth
    flipped = A.bilinear(img, pts_uv[:, 0], 1.0 - pts_uv[:, 1]) / 255.0
    assert np.abs(flipped - (0.5 + 0.4 * pts)).max() > 10 / 255


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_store_matches_field(dtype_guard, fp16):
    from customnerf_amd import mesh
    model = gaussian_model(dtype_guard, fp16)
    m = model.extract_mesh(resolution=40, threshold=10.0, aabb=AABB)
    v, f, n = m['verts'], m['faces'], m['normals']
    F = f.shape[0]
    Rr = 256
    _, s = A.layout(F, Rr)
    seen = []

    def color_fn(x, d):
        rgbc = model(x, d)[1]
        seen.append((x.clone(), d.clone(), rgbc.clone()))
        return rgbc                                                                # [N, 4] (rgb + confidence): the first three are used

    fill = (1, 2, 3)
    uvs, tex = mesh.bake_texture(v, f, Rr, color_fn, normals=n, chunk=20_000, fill=fill)
    total = (F + 1) // 2 * s * s
    assert sum(len(a[0]) for a in seen) == total and len(seen) == -(-total // 20_000)
    x = torch.cat([a[0] for a in seen]).cpu().numpy()
    d = torch.cat([a[1] for a in seen]).cpu().numpy()
    rgb = torch.cat([a[2] for a in seen])[:, :3].float().clamp(0, 1)
    want = (rgb * 255).round().to(torch.uint8).cpu().numpy()
    xr, dr = A.points(v.cpu().numpy(), f.cpu().numpy(), Rr, normals=n.cpu().numpy())
    np.testing.assert_array_equal(x.view(np.uint32), xr.view(np.uint32))
    np.testing.assert_allclose(d, dr, rtol=0, atol=2e-6)
    face, _, _, X, Y = A.cell_texels(F, Rr)
    t = tex.cpu().numpy()
    own = face >= 0
    np.testing.assert_array_equal(t[Y[own], X[own]], want[own])
    own_map = A.owner_map(F, Rr)
    assert (t[own_map < 0] == fill).all()
    np.testing.assert_array_equal(uvs.cpu().numpy().view(np.uint32), A.uvs(F, Rr).view(np.uint32))


def test_save_mesh_textured_obj(dtype_guard, tmp_path):
    model = gaussian_model(dtype_guard, False)
    kw = dict(resolution=96, threshold=10.0, aabb=AABB, keep_largest=True, target_faces=1000)
    mp = model.save_mesh(str(tmp_path / "blob.ply"), color=True, **kw)
    mo = model.save_mesh(str(tmp_path / "blob.obj"), texture=256, **kw)
    assert mp['uvs'] is None and mp['texture'] is None
    ply = R.read_ply(str(tmp_path / "blob.ply"))
    o = A.read_obj(str(tmp_path / "blob.obj"))
    assert o["mtllib"] == "blob.mtl" and "map_Kd blob.png" in open(str(tmp_path / "blob.mtl")).read()
    assert np.array_equal(o["verts"], ply["verts"]) and np.array_equal(o["f"][..., 0] - 1, ply["faces"])      # the PLY path's geometry
    assert np.array_equal(o["normals"], ply["normals"]) and np.array_equal(o["f"][..., 2] - 1, ply["faces"])
    F = len(ply["faces"])
    assert F in (999, 1000)
    img = A.read_png(str(tmp_path / "blob.png"))
    assert img.shape == (256, 256, 3)
    np.testing.assert_array_equal(img, mo['texture'].cpu().numpy())
    np.testing.assert_array_equal(o["uvs"].reshape(-1, 3, 2), mo['uvs'].cpu().numpy())
    # the texel under each face corner is that vertex's colour (same point; the direction renormalised) within one step
    XY = A.corner_texels(F, 256)
    corner_rgb = img[XY[..., 1], XY[..., 0]].astype(np.int32)                          # [F, 3, 3]
    vert_rgb = ply["colors"][ply["faces"]].astype(np.int32)
    assert np.abs(corner_rgb - vert_rgb).max() <= 1
    own = A.owner_map(F, 256)
    assert (img[own < 0] == 0).all()                                                  # default fill on exactly the un-owned texels
    assert (img[own >= 0].max(axis=1) > 0).mean() > 0.99
    with pytest.raises(ValueError, match=r"\.obj"):
        model.save_mesh(str(tmp_path / "blob2.ply"), texture=256, **kw)
    with pytest.raises(ValueError, match="decimate"):
        model.extract_mesh(resolution=48, threshold=10.0, aabb=AABB, texture=16)      # thousands of faces on 16 x 16 texels
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=16, aabb=AABB, texture=-1)


def test_edge_cases():
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib, ptr, stream
    v, f, n = (cuda(a) for a in sphere_mesh(14))                              # 1340 faces: cells of 4 texels at R = 128
    F = f.shape[0]
    # F = 0: no UV, everything is fill
    uvs, tex = mesh.bake_texture(v, f[:0], 32, lambda x, d: x, fill=(9, 8, 7))
    assert uvs.shape == (0, 3, 2) and (tex.cpu().numpy() == (9, 8, 7)).all()
    # F = 1: one cell of R texels; B is un-owned
    uvs, tex = mesh.bake_texture(v, f[:1], 16, lambda x, d: torch.full_like(x, 0.5), fill=(9, 8, 7))
    t = tex.cpu().numpy()
    own = A.owner_map(1, 16)
    assert (t[own == 0] == 128).all() and (t[own < 0] == (9, 8, 7)).all() and (own == 0).sum() == 16 * 17 // 2
    np.testing.assert_array_equal(uvs.cpu().numpy(), A.uvs(1, 16))
    # capacities: entries past max_faces / max_points are not written
    Rr = 128
    uvs, flags = atlas_uvs(v, f, Rr, max_faces=F // 2)
    u = uvs.cpu().numpy()
    np.testing.assert_array_equal(u[:F // 2], A.uvs(F, Rr)[:F // 2])
    assert (u[F // 2:] == -7.0).all()
    x, d = atlas_points(v, f, n, Rr, flags, 5, 500, max_points=100)
    xr, dr = A.points(v.cpu().numpy(), f.cpu().numpy(), Rr, normals=n.cpu().numpy(), t0=5, t1=500)
    np.testing.assert_array_equal(x[:100].cpu().numpy(), xr[:100])
    assert (x[100:].cpu().numpy() == -7.0).all() and (d[100:].cpu().numpy() == -7.0).all()
    # an index out of range: ValueError; the flag stops points and store from writing anything
    bad = f.clone()
    bad[F // 3, 1] = v.shape[0]
    with pytest.raises(ValueError, match="outside"):
        mesh.bake_texture(v, bad, Rr, lambda x, d: x)
    bad[F // 3, 1] = -1
    with pytest.raises(ValueError, match="outside"):
        mesh.bake_texture(v, bad, Rr, lambda x, d: x)
    _, flags = atlas_uvs(v, bad, Rr)
    assert int(flags.cpu()[0]) == 1
    x, d = atlas_points(v, bad, n, Rr, flags, 0, 1000)
    assert (x.cpu().numpy() == -7.0).all() and (d.cpu().numpy() == -7.0).all()
    img = torch.full((Rr, Rr, 3), 77, dtype=torch.uint8, device="cuda")
    rgb = torch.rand(1000, 3, device="cuda")
    assert lib.cnerf_mesh_atlas_store(F, Rr, 0, 1000, ptr(rgb), 3, (C.c_uint8 * 3)(1, 2, 3), ptr(flags), ptr(img), stream()) == 0
    assert (img.cpu().numpy() == 77).all()
    # arguments the library rejects before any launch
    _, s = A.layout(F, Rr)
    assert lib.cnerf_mesh_atlas_points(ptr(v), None, v.shape[0], ptr(f), F, Rr, 0, (F + 1) // 2 * s * s + 1, ptr(flags), ptr(x), ptr(d),
                                       10, stream()) == -1
    assert lib.cnerf_mesh_atlas_store(F, Rr, 0, 10, ptr(rgb), 2, (C.c_uint8 * 3)(), ptr(flags), ptr(img), stream()) == -1
    assert lib.cnerf_mesh_atlas_uvs(ptr(f), v.shape[0], F, 15, None, 0, ptr(flags), stream()) == -1
    # a resolution too small for F, and a color_fn of the wrong shape
    with pytest.raises(ValueError, match="decimate"):
        mesh.bake_texture(v, f, 16, lambda x, d: x)
    with pytest.raises(ValueError, match="color_fn"):
        mesh.bake_texture(v, f, Rr, lambda x, d: x[:, :2])
    # a half-precision, wider color_fn output is read through its first three columns
    _, t16 = mesh.bake_texture(v, f, Rr, lambda x, d: torch.cat([0.5 + 0.4 * x, x[:, :2]], 1).half(), normals=n)
    _, t32 = mesh.bake_texture(v, f, Rr, lambda x, d: (0.5 + 0.4 * x).half().float(), normals=n)
    assert torch.equal(t16, t32)
