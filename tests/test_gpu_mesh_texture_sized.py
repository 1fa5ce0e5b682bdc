"""GPU: the area-proportional texture atlas (csrc/mesh_texture.hip, cnerf_mesh_atlas_sized_*) against its NumPy restatement
(tests/atlas_sized_restatement.py) — threshold, counts, cells, UVs and points bit-equal, directions to 2e-6 — a colour affine in position
reproduced by bilinear lookup of the written PNG through the written OBJ's UVs, the store against the field's own colours, end to end through
NeRFRenderer.save_mesh(..., texture_layout='area') and render_mesh, and the uniform layout left bit for bit as it was."""
import ctypes as C
import functools
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
import atlas_sized_restatement as S  # noqa: E402
import atlas_sized_testlib as T  # noqa: E402
import raster_restatement as RS  # noqa: E402
from mesh_testlib import AABB, cuda, dtype_guard, gaussian_model  # noqa: E402,F401

PAD = -7


@functools.lru_cache(maxsize=None)
def decimated_sphere():
    """the 40^3 sphere decimated to about 300 faces (large faces where it is flat, small ones where the lattice left slivers)"""
    from customnerf_amd import mesh
    v, f, n = T.sphere_mesh()
    dv, df, dn, _ = mesh.decimate(cuda(v), cuda(f), 300, normals=cuda(n))
    return dv.cpu().numpy(), df.cpu().numpy(), dn.cpu().numpy()


def meshes():
    v, f, n, _ = T.hand_soup()
    yield "hand_soup", (lambda: (v, f, n)), 64, None
    yield "hand_soup_e1080", (lambda: (v, f, n)), 64, 1080                    # the threshold 16 keys under the bin boundary of the 32-long edge
    yield "hand_soup_no_normals", (lambda: (v, f, None)), 128, None
    yield "decimated_sphere", decimated_sphere, 256, None
    yield "torus", T.torus_mesh, 2048, None
    yield "empty", (lambda: (v, f[:0], n)), 32, None


MESHES = list(meshes())


def sized_run(v, f, n, Rr, e=None, counts=None, max_faces=None, t0=0, t1=None, max_points=None):
    """the passes through the C ABI -> dict of host arrays; cells, uvs, x and d are padded by 8 rows of PAD.  Without e: the threshold and
    counts of the library's layout; with e: that threshold, and its counts from the histogram read back unless `counts` gives them."""
    from customnerf_amd._lib import lib, check, ptr, stream
    V, F = v.shape[0], f.shape[0]
    nbytes = C.c_uint64(0)
    check(lib.cnerf_mesh_atlas_sized_workspace_bytes(F, C.byref(nbytes)), "bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    hist = torch.full((2049,), 0x55, dtype=torch.int32, device="cuda")
    check(lib.cnerf_mesh_atlas_sized_measure(ptr(v), V, ptr(f) if F else None, F, ptr(ws), nbytes.value, ptr(hist), stream()), "measure")
    h = hist.cpu().numpy().astype(np.int64)
    out = dict(hist=h[:2048], flags=int(h[2048]))
    ee, tiles = C.c_uint32(0), C.c_uint32(0)
    if e is None:
        counts = (C.c_uint32 * 8)()
        check(lib.cnerf_mesh_atlas_sized_layout((C.c_uint32 * 2048)(*h[:2048].tolist()), Rr, C.byref(ee), counts, C.byref(tiles)), "layout")
    else:                                                                      # another threshold that fits
        nn = S.class_counts(h[:2048], e, S.classes_of(Rr)) if counts is None else counts
        ee, tiles, counts = C.c_uint32(e), C.c_uint32(S.tiles_of(nn)), (C.c_uint32 * 8)(*[int(c) for c in nn])
    out.update(e=ee.value, tiles=tiles.value, counts=np.array(list(counts), np.int64))
    flags = hist[2048:]
    cells = torch.full((F + 8, 4), PAD, dtype=torch.int32, device="cuda")
    mf = F if max_faces is None else max_faces
    check(lib.cnerf_mesh_atlas_sized_plan(F, Rr, ee.value, counts, ptr(ws), nbytes.value, ptr(flags), ptr(cells), mf, stream()), "plan")
    uvs = torch.full((F + 8, 3, 2), float(PAD), device="cuda")
    check(lib.cnerf_mesh_atlas_sized_uvs(F, Rr, ptr(cells), ptr(flags), ptr(uvs), mf, stream()), "uvs")
    t1 = 16 * tiles.value if t1 is None else t1
    N = t1 - t0
    x = torch.full((N + 8, 3), float(PAD), device="cuda")
    d = torch.full((N + 8, 3), float(PAD), device="cuda")
    check(lib.cnerf_mesh_atlas_sized_points(ptr(v), ptr(n), V, ptr(f) if F else None, F, Rr, counts, ptr(ws), nbytes.value, t0, t1, ptr(flags),
                                            ptr(x), ptr(d), N if max_points is None else max_points, stream()), "points")
    out.update(cells=cells.cpu().numpy(), uvs=uvs.cpu().numpy(), x=x.cpu().numpy(), d=d.cpu().numpy(), ws=ws, counts_c=counts, nbytes=nbytes.value,
               flags_dev=flags)
    return out


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name,get,Rr,e", MESHES, ids=[m[0] for m in MESHES])
def test_plan_uvs_and_points_match_restatement(name, get, Rr, e):
    v, f, n = get()
    F = len(f)
    p = S.plan(v, f, Rr, e=e)
    gv, gf, gn = cuda(v), cuda(f), cuda(n)
    runs = [sized_run(gv, gf, gn, Rr, e=e) for _ in range(2)]
    r = runs[0]
    total = p.texels
    print(f"{name}: F = {F}, e = {p.e}, counts {p.n.tolist()}, tiles {p.tiles} of {(Rr // 4) ** 2}")
    assert r["flags"] == 0
    np.testing.assert_array_equal(r["hist"], p.hist)
    assert (r["e"], r["tiles"]) == (p.e, p.tiles)
    np.testing.assert_array_equal(r["counts"], p.n)
    np.testing.assert_array_equal(r["cells"][:F], p.cells)
    np.testing.assert_array_equal(r["uvs"][:F].view(np.uint32), S.uvs(p).view(np.uint32))
    assert (r["cells"][F:] == PAD).all() and (r["uvs"][F:] == PAD).all() and (r["x"][total:] == PAD).all() and (r["d"][total:] == PAD).all()
    # every cell texel of a small atlas; of a large one the first and last texels and those around every class boundary (the restatement is slow)
    cuts = sorted({0, total} | {int(16 * o) for o in p.O})
    spans = [(0, total)] if total <= 400_000 else sorted({(max(0, c - 60_000), min(total, c + 60_000)) for c in cuts})
    for a, b in spans:
        xr, dr = S.points(p, v, f, normals=n, t0=a, t1=b)
        assert len(xr) == b - a
        np.testing.assert_array_equal(r["x"][a:b].view(np.uint32), xr.view(np.uint32))
        np.testing.assert_allclose(r["d"][a:b], dr, rtol=0, atol=2e-6)
    if total:
        np.testing.assert_allclose(np.linalg.norm(r["d"][:total], axis=1), 1.0, atol=1e-6)
    for key in ("hist", "cells", "uvs", "x", "d"):                             # a second run is bit-identical
        np.testing.assert_array_equal(bits(r[key]), bits(runs[1][key]))
    if not total:
        return
    # a split [t0, t1) that crosses a class boundary equals the whole range
    edges = sorted({int(16 * o) for o in p.O if 0 < 16 * o < total})
    assert edges or len(np.nonzero(p.n)[0]) == 1
    mid = edges[len(edges) // 2] if edges else total // 2
    t0, t1 = max(0, mid - 37), min(total, mid + 301)
    c = sized_run(gv, gf, gn, Rr, e=e, t0=t0, t1=t1)
    np.testing.assert_array_equal(bits(c["x"][:t1 - t0]), bits(r["x"][t0:t1]))
    np.testing.assert_array_equal(bits(c["d"][:t1 - t0]), bits(r["d"][t0:t1]))
    assert (c["x"][t1 - t0:] == PAD).all()


def test_hand_soup_is_the_mesh_it_should_be():
    """four classes, one with an odd count (an un-owned B), one with a single face, and the degenerate faces in class 0"""
    v, f, n, names = T.hand_soup()
    r = sized_run(cuda(v), cuda(f), cuda(n), 64)
    present = r["counts"][r["counts"] > 0]
    assert len(present) >= 4 and (present % 2 == 1).any() and (present == 1).any()
    for name in ("zero_area", "zero_length", "denormal", "overflow"):
        assert r["cells"][names[name], 2] == 4, name
    r = sized_run(cuda(v), cuda(f), cuda(n), 64, e=1080)
    assert r["cells"][names["boundary"], 2] == 8 and r["cells"][names["below_boundary"], 2] == 4


def test_capacities_and_bad_index():
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib, ptr, stream
    v, f, n = decimated_sphere()
    F, Rr = len(f), 256
    gv, gf, gn = cuda(v), cuda(f), cuda(n)
    p = S.plan(v, f, Rr)
    # rows past max_faces and max_points are left untouched
    r = sized_run(gv, gf, gn, Rr, max_faces=F // 2, t0=5, t1=5000, max_points=100)
    np.testing.assert_array_equal(r["cells"][:F // 2], p.cells[:F // 2])
    np.testing.assert_array_equal(r["uvs"][:F // 2], S.uvs(p)[:F // 2])
    assert (r["cells"][F // 2:] == PAD).all() and (r["uvs"][F // 2:] == PAD).all()
    xr, _ = S.points(p, v, f, normals=n, t0=5, t1=5000)
    np.testing.assert_array_equal(r["x"][:100], xr[:100])
    assert (r["x"][100:] == PAD).all() and (r["d"][100:] == PAD).all()
    # arguments the library rejects before any launch
    one = torch.zeros(64, device="cuda")
    assert lib.cnerf_mesh_atlas_sized_points(ptr(gv), None, len(v), ptr(gf), F, Rr, r["counts_c"], ptr(r["ws"]), r["nbytes"], 0, p.texels + 1,
                                             ptr(r["flags_dev"]), ptr(one), ptr(one), 1, stream()) == -1
    assert lib.cnerf_mesh_atlas_sized_store(F, Rr, r["counts_c"], ptr(r["ws"]), r["nbytes"], 0, 10, ptr(one), 2, (C.c_uint8 * 3)(),
                                            ptr(r["flags_dev"]), ptr(one), stream()) == -1
    # an index out of range: the flag is set and plan, uvs, points and store write nothing; bake_texture raises
    for badv in (len(v), -1):
        bad = gf.clone()
        bad[F // 3, 1] = badv
        r = sized_run(gv, bad, gn, Rr, e=p.e, counts=p.n)                     # a plan that is valid for F faces: the flag alone stops the passes
        assert r["flags"] == 1
        assert (r["cells"] == PAD).all() and (r["uvs"] == PAD).all() and (r["x"] == PAD).all() and (r["d"] == PAD).all()
        img = torch.full((Rr, Rr, 3), 77, dtype=torch.uint8, device="cuda")
        rgb = torch.rand(1000, 3, device="cuda")
        assert lib.cnerf_mesh_atlas_sized_store(F, Rr, r["counts_c"], ptr(r["ws"]), r["nbytes"], 0, 1000, ptr(rgb), 3, (C.c_uint8 * 3)(1, 2, 3),
                                                ptr(r["flags_dev"]), ptr(img), stream()) == 0
        assert (img.cpu().numpy() == 77).all()
        with pytest.raises(ValueError, match="outside"):
            mesh.bake_texture(gv, bad, Rr, lambda x, d: x, layout='area')
        with pytest.raises(ValueError, match="outside"):
            mesh.atlas_plan(gv, bad, Rr)


def test_atlas_plan_members():
    from customnerf_amd import mesh
    v, f, n = decimated_sphere()
    p = S.plan(v, f, 256)
    a = mesh.atlas_plan(cuda(v), cuda(f), 256)
    assert (a.resolution, a.e, a.tiles, a.texels) == (256, p.e, p.tiles, p.texels) and a.counts == p.n[:p.K + 1].tolist()
    assert a.threshold == S.threshold(p.e) and isinstance(a.threshold, float)
    assert a.cells.dtype == torch.int32 and a.cells.is_cuda
    np.testing.assert_array_equal(a.cells.cpu().numpy(), p.cells)
    e = mesh.atlas_plan(cuda(v), cuda(f[:0]), 64)
    assert (e.e, e.tiles, e.texels, e.counts) == (0, 0, 0, [0] * 5) and tuple(e.cells.shape) == (0, 4)


def test_affine_colour_bake(tmp_path):
    """colour = 0.5 + 0.4 x baked with layout='area' on the decimated sphere, written (OBJ + PNG), read back: bilinear lookup at random
    points of every UV triangle gives the colour of the surface point within the uint8 rounding, in every class of cell"""
    from customnerf_amd import mesh
    v, f, n = decimated_sphere()
    Rr = 256
    p = S.plan(v, f, Rr)
    assert len(np.nonzero(p.n)[0]) >= 2                                        # more than one cell size
    uvs, tex = mesh.bake_texture(cuda(v), cuda(f), Rr, lambda x, d: 0.5 + 0.4 * x, normals=cuda(n), chunk=10_000, layout='area')
    path = str(tmp_path / "affine.obj")
    mesh.write_obj(path, v, f, uvs=uvs, normals=n, texture=tex)
    o = A.read_obj(path)
    img = A.read_png(str(tmp_path / "affine.png"))
    np.testing.assert_array_equal(img, tex.cpu().numpy())
    assert np.array_equal(o["verts"], v) and np.array_equal(o["f"][..., 0] - 1, f)
    uv = o["uvs"][o["f"][..., 1] - 1].astype(np.float64)
    np.testing.assert_array_equal(o["uvs"].reshape(-1, 3, 2), S.uvs(p))
    rng = np.random.default_rng(0)
    w = np.concatenate([np.eye(3), [[0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]], rng.dirichlet((1, 1, 1), 40)])
    pts_uv = np.einsum("kc,fcd->fkd", w, uv).reshape(-1, 2)
    pts = np.einsum("kc,fcd->fkd", w, v[f].astype(np.float64)).reshape(-1, 3)
    got = A.bilinear(img, pts_uv[:, 0], pts_uv[:, 1]) / 255.0
    err = np.abs(got - (0.5 + 0.4 * pts))
    print(f"counts {p.n.tolist()}: worst colour error {err.max() * 255:.4f} levels (bound 0.6)")
    assert err.max() <= 0.6 / 255, err.max()
    flipped = A.bilinear(img, pts_uv[:, 0], 1.0 - pts_uv[:, 1]) / 255.0                 # a v-flipped lookup would not pass
    assert np.abs(flipped - (0.5 + 0.4 * pts)).max() > 10 / 255


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_store_matches_field(dtype_guard, fp16):
    from customnerf_amd import mesh
    model = gaussian_model(dtype_guard, fp16)
    m = model.extract_mesh(resolution=40, threshold=10.0, aabb=AABB)
    v, f, n = m['verts'], m['faces'], m['normals']
    Rr = 256
    vh, fh, nh = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    p = S.plan(vh, fh, Rr)
    seen = []

    def color_fn(x, d):
        rgbc = model(x, d)[1]
        seen.append((x.clone(), d.clone(), rgbc.clone()))
        return rgbc                                                                # [N, 4]: the first three are used

    fill = (1, 2, 3)
    uvs, tex = mesh.bake_texture(v, f, Rr, color_fn, normals=n, chunk=20_000, fill=fill, layout='area')
    total = p.texels
    assert sum(len(a[0]) for a in seen) == total and len(seen) == -(-total // 20_000)
    x = torch.cat([a[0] for a in seen]).cpu().numpy()
    d = torch.cat([a[1] for a in seen]).cpu().numpy()
    rgb = torch.cat([a[2] for a in seen])[:, :3].float().clamp(0, 1)
    want = (rgb * 255).round().to(torch.uint8).cpu().numpy()
    xr, dr = S.points(p, vh, fh, normals=nh)
    np.testing.assert_array_equal(x.view(np.uint32), xr.view(np.uint32))
    np.testing.assert_allclose(d, dr, rtol=0, atol=2e-6)
    face, _, _, X, Y, _ = S.cell_texels(p)
    t = tex.cpu().numpy()
    own = face >= 0
    np.testing.assert_array_equal(t[Y[own], X[own]], want[own])                    # every owned texel: the rounded colour
    own_map = S.owner_map(p)
    assert (own_map >= 0).sum() == own.sum()
    assert (t[own_map < 0] == fill).all()                                          # every other texel: the fill
    np.testing.assert_array_equal(uvs.cpu().numpy().view(np.uint32), S.uvs(p).view(np.uint32))


def test_save_mesh_area_layout_and_render(dtype_guard, tmp_path):
    from customnerf_amd import scene
    model = gaussian_model(dtype_guard, False)
    kw = dict(resolution=96, threshold=10.0, aabb=AABB, keep_largest=True, target_faces=1000)
    mo = model.save_mesh(str(tmp_path / "blob.obj"), texture=256, texture_layout='area', **kw)
    assert mo['texture_layout'] == 'area'
    o = A.read_obj(str(tmp_path / "blob.obj"))
    assert o["mtllib"] == "blob.mtl" and "map_Kd blob.png" in open(str(tmp_path / "blob.mtl")).read()
    img = A.read_png(str(tmp_path / "blob.png"))
    assert img.shape == (256, 256, 3)
    np.testing.assert_array_equal(img, mo['texture'].cpu().numpy())
    v, f = mo['verts'].cpu().numpy(), mo['faces'].cpu().numpy()
    assert np.array_equal(o["verts"], v) and np.array_equal(o["f"][..., 0] - 1, f) and len(f) in (999, 1000)
    p = S.plan(v, f, 256)
    uv = mo['uvs'].cpu().numpy()
    np.testing.assert_array_equal(uv.view(np.uint32), S.uvs(p).view(np.uint32))
    np.testing.assert_array_equal(o["uvs"].reshape(-1, 3, 2), uv)
    own = S.owner_map(p)
    assert (img[own < 0] == 0).all() and (img[own >= 0].max(axis=1) > 0).mean() > 0.99
    # the preview of the export is the shade restatement's, fed the same uvs and texture
    H = W = 128
    pose, intr = scene.camera_pose(3, radius=1.2), scene.intrinsics(H, W)
    image, mask, _ = model.render_mesh(mo, pose, intr, H, W)
    vis = RS.visibility(v, f, pose, intr, H, W)
    want, wmask = RS.shade(vis, v, f, 'texture', uvs=uv, texture=img)
    got = image.cpu().numpy()
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{int((diff > 0).sum())} of {diff.size} values differ, worst {int(diff.max())}; {int((wmask > 0).sum())} pixels hit")
    assert (wmask > 0).sum() > 1000
    np.testing.assert_array_equal(mask.cpu().numpy(), wmask > 0)
    np.testing.assert_array_equal(got, want)
    # the default layout says so in the dict
    assert model.extract_mesh(resolution=24, threshold=10.0, aabb=AABB)['texture_layout'] == 'uniform'


def test_uniform_layout_is_unchanged():
    """layout='uniform' and the default give what the uniform passes give when called one by one, as bake_texture called them before the
    layout argument existed: the same tensors, bit for bit"""
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib, check, ptr, stream
    v, f, n = (cuda(a) for a in T.sphere_mesh())
    V, F, Rr = v.shape[0], f.shape[0], 512
    color_fn = lambda x, d: 0.5 + 0.4 * x + 0.1 * d                               # noqa: E731
    fill = (C.c_uint8 * 3)(4, 5, 6)
    uvs = torch.empty(F, 3, 2, device="cuda")
    flags = torch.empty(1, dtype=torch.int32, device="cuda")
    check(lib.cnerf_mesh_atlas_uvs(ptr(f), V, F, Rr, ptr(uvs), F, ptr(flags), stream()), "uvs")
    tex = torch.empty(Rr, Rr, 3, dtype=torch.uint8, device="cuda")
    check(lib.cnerf_mesh_atlas_fill(F, Rr, fill, ptr(tex), stream()), "fill")
    _, s = A.layout(F, Rr)
    total = (F + 1) // 2 * s * s
    x, d = torch.empty(total, 3, device="cuda"), torch.empty(total, 3, device="cuda")
    check(lib.cnerf_mesh_atlas_points(ptr(v), ptr(n), V, ptr(f), F, Rr, 0, total, ptr(flags), ptr(x), ptr(d), total, stream()), "points")
    rgb = color_fn(x, d).contiguous()
    check(lib.cnerf_mesh_atlas_store(F, Rr, 0, total, ptr(rgb), 3, fill, ptr(flags), ptr(tex), stream()), "store")
    np.testing.assert_array_equal(uvs.cpu().numpy().view(np.uint32), A.uvs(F, Rr).view(np.uint32))
    for kw in ({}, {"layout": "uniform"}):
        u2, t2 = mesh.bake_texture(v, f, Rr, color_fn, normals=n, chunk=300_000, fill=(4, 5, 6), **kw)
        assert torch.equal(u2.view(torch.int32), uvs.view(torch.int32)) and torch.equal(t2, tex), kw


def test_value_errors():
    from customnerf_amd import mesh
    v, f, n = (cuda(a) for a in T.sphere_mesh())
    with pytest.raises(ValueError, match="layout"):
        mesh.bake_texture(v, f, 512, lambda x, d: x, layout='charts')
    for Rr in (500, 48, 8, 32768):
        with pytest.raises(ValueError, match="power of two"):
            mesh.bake_texture(v, f, Rr, lambda x, d: x, layout='area')
        with pytest.raises(ValueError, match="power of two"):
            mesh.atlas_plan(v, f, Rr)
    with pytest.raises(ValueError, match="decimate the mesh"):                   # 11516 faces need 5758 cells; 128 x 128 texels hold 1024
        mesh.bake_texture(v, f, 128, lambda x, d: x, layout='area')
    with pytest.raises(ValueError, match="decimate the mesh"):
        mesh.atlas_plan(v, f[:33], 16)
    assert mesh.atlas_plan(v, f[:32], 16).counts == [32, 0, 0]
    with pytest.raises(ValueError, match="color_fn"):
        mesh.bake_texture(v, f[:32], 16, lambda x, d: x[:, :2], layout='area')
