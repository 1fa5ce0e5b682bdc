"""GPU: the chart-based texture atlas (csrc/mesh_charts.hip, cnerf_mesh_atlas_proj_*) against its NumPy restatement
(tests/atlas_proj_restatement.py) — classes, charts, extents, density, rectangles, UVs, both owner maps, the texel count and the points
bit-equal, directions to 2e-6 — a colour affine in position reproduced by bilinear lookup of the written PNG through the written OBJ's UVs
on the meshes with planar charts, the texture of a curved mesh bit-equal to the restatement's, the store against the field's own colours,
baking from a source with a normal map, and end to end through NeRFRenderer.save_mesh(..., texture_layout='projected') and render_mesh."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import atlas_restatement as A  # noqa: E402
import atlas_proj_restatement as P  # noqa: E402
import atlas_proj_testlib as T  # noqa: E402
import raster_restatement as RS  # noqa: E402
from mesh_testlib import AABB, cuda, dtype_guard, gaussian_model  # noqa: E402,F401

PAD = -7
f32 = np.float32


decimated_sphere = T.decimated_sphere


def soup():
    v, f, n, _ = T.hand_soup()
    return v, f, n


def empty():
    v, f, n, _ = T.hand_soup()
    return v, f[:0], n


# name, mesh, resolution, gutters
MESHES = [("hand_soup", soup, 64, (0, 2, 8)), ("cube", T.cube, 64, (2,)), ("quad", T.quad, 512, (0, 2, 8)),
          ("quad_at_threshold", T.quad, 36, (2,)), ("quad_over_threshold", T.quad, 37, (2,)),       # boxes of 32^2 = 1024 and 33^2 texels
          ("sphere", T.sphere_mesh, 512, (2,)),
          ("decimated_sphere", decimated_sphere, 256, (2,)), ("torus", T.torus_mesh, 1024, (2,)), ("empty", empty, 32, (2,))]
CASES = [pytest.param(get, R, g, id=f"{name}-g{g}") for name, get, R, gs in MESHES for g in gs]
_PLANS = {}


def plan_of(get, R, g):
    key = (get, R, g)
    if key not in _PLANS:
        v, f, n = get()
        _PLANS[key] = P.plan(v, f, R, n, g)
    return _PLANS[key]


def proj_run(v, f, n, Rr, g, max_faces=None, max_charts=None, t0=0, t1=None, max_points=None, pack=True):
    """the passes through the C ABI -> dict of host arrays; per-face and per-texel outputs are padded by 8 rows of PAD"""
    from customnerf_amd._lib import lib, check, ptr, stream
    v, f, n = cuda(np.asarray(v, f32)), cuda(np.asarray(f, np.int32)), cuda(n)
    V, F = v.shape[0], f.shape[0]
    mf = F if max_faces is None else max_faces
    nbytes = C.c_uint64(0)
    check(lib.cnerf_mesh_atlas_proj_workspace_bytes(V, F, Rr, C.byref(nbytes)), "bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), 0x55, dtype=torch.int32, device="cuda")
    fclass = torch.full((F + 8,), PAD, dtype=torch.int32, device="cuda")
    fchart = torch.full((F + 8,), PAD, dtype=torch.int32, device="cuda")
    ext = torch.full((F + 8, 4), float(PAD), dtype=torch.float32, device="cuda")
    fp = ptr(f) if F else None
    check(lib.cnerf_mesh_atlas_proj_charts(ptr(v), None if n is None else ptr(n), V, fp, F, Rr, ptr(ws), nbytes.value, ptr(counts),
                                           ptr(fclass), ptr(fchart), mf, ptr(ext), F if max_charts is None else max_charts, stream()), "charts")
    nc, flag = (int(c) for c in counts.cpu())
    out = dict(C=nc, flags=flag, face_class=fclass.cpu().numpy(), face_chart=fchart.cpu().numpy(), extents=ext.cpu().numpy())
    if not pack:
        nc = 0
    e = np.ascontiguousarray(out["extents"][:nc])
    rho = C.c_double(0.0)
    rects = np.zeros((nc, 4), np.int32)
    check(lib.cnerf_mesh_atlas_proj_pack(e.ctypes.data_as(C.c_void_p), nc, Rr, g, C.byref(rho), rects.ctypes.data_as(C.c_void_p)), "pack")
    rd = cuda(rects)
    uvs = torch.full((F + 8, 3, 2), float(PAD), dtype=torch.float32, device="cuda")
    own_ab = torch.full((Rr, Rr), PAD, dtype=torch.int32, device="cuda")
    own = torch.full((Rr, Rr), PAD, dtype=torch.int32, device="cuda")
    totals = torch.full((2,), PAD, dtype=torch.int64, device="cuda")
    flags = counts[1:]
    check(lib.cnerf_mesh_atlas_proj_raster(ptr(v), V, fp, F, Rr, g, rho.value, ptr(rd) if nc else None, nc, ptr(ws), nbytes.value, ptr(flags),
                                           ptr(uvs), mf, ptr(own_ab), ptr(own), ptr(totals), stream()), "raster")
    total, overlap = (int(t) for t in totals.cpu())
    t1 = total if t1 is None else t1
    N = t1 - t0
    x = torch.full((N + 8, 3), float(PAD), dtype=torch.float32, device="cuda")
    d = torch.full((N + 8, 3), float(PAD), dtype=torch.float32, device="cuda")
    check(lib.cnerf_mesh_atlas_proj_points(ptr(v), None if n is None else ptr(n), V, fp, F, Rr, ptr(ws), nbytes.value, t0, t1, ptr(flags),
                                           ptr(x), ptr(d), N if max_points is None else max_points, stream()), "points")
    rgb = torch.rand(max(N, 1), 3, device="cuda")
    img = torch.full((Rr, Rr, 3), 77, dtype=torch.uint8, device="cuda")
    check(lib.cnerf_mesh_atlas_proj_store(V, F, Rr, ptr(ws), nbytes.value, t0, t1, ptr(rgb), 3, ptr(flags), ptr(img), stream()), "store")
    check(lib.cnerf_mesh_atlas_proj_fill(V, F, Rr, ptr(ws), nbytes.value, (C.c_uint8 * 3)(9, 8, 7), ptr(flags), ptr(img), stream()), "fill")
    out.update(rho=rho.value, rects=rects, uvs=uvs.cpu().numpy(), owner_ab=own_ab.cpu().numpy(), owner=own.cpu().numpy(), total=total,
               overlap=overlap, x=x.cpu().numpy(), d=d.cpu().numpy(), rgb=rgb.cpu().numpy(), image=img.cpu().numpy())
    return out


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_decimated_sphere_is_what_decimate_gives():
    """the stored mesh is mesh.decimate's output on the 40^3 sphere, bit for bit: the CPU tests check the layout's invariants on the mesh
    the device would make today"""
    from customnerf_amd import mesh
    v, f, n = T.sphere_mesh()
    dv, df, dn, _ = mesh.decimate(cuda(v), cuda(f), 300, normals=cuda(n))
    sv, sf, sn = decimated_sphere()
    assert len(sf) == 300
    np.testing.assert_array_equal(df.cpu().numpy(), sf)
    np.testing.assert_array_equal(bits(dv.cpu().numpy()), bits(sv))
    np.testing.assert_array_equal(bits(dn.cpu().numpy()), bits(sn))


@pytest.mark.parametrize("get,Rr,g", CASES)
def test_matches_restatement(get, Rr, g):
    v, f, n = get()
    F = len(f)
    p = plan_of(get, Rr, g)
    got = proj_run(v, f, n, Rr, g)
    assert got["flags"] == 0 and got["C"] == p.C
    np.testing.assert_array_equal(got["face_class"][:F], p.classes)
    np.testing.assert_array_equal(got["face_chart"][:F], p.face_chart)
    np.testing.assert_array_equal(bits(got["extents"][:p.C]), bits(p.extents))
    assert struct.pack("<d", got["rho"]) == struct.pack("<d", p.rho)
    np.testing.assert_array_equal(got["rects"], p.rects)
    np.testing.assert_array_equal(bits(got["uvs"][:F]), bits(p.uvs))
    np.testing.assert_array_equal(got["owner_ab"], p.owner_ab)
    np.testing.assert_array_equal(got["owner"], p.owner)
    assert (got["total"], got["overlap"]) == (p.total, p.overlap)
    xr, dr = P.points(p, v, f, n)
    np.testing.assert_array_equal(bits(got["x"][:p.total]), bits(xr))
    np.testing.assert_allclose(got["d"][:p.total], dr, rtol=0, atol=2e-6)
    # rows past the capacities were given are untouched
    for k in ("face_class", "face_chart", "extents", "uvs", "x", "d"):
        tail = got[k][{"extents": p.C, "x": p.total, "d": p.total}.get(k, F):]
        assert (tail == PAD).all(), k
    # the store and the fill
    img = got["image"]
    want = np.rint(np.clip(got["rgb"][:p.total], 0, 1) * f32(255)).astype(np.uint8)
    np.testing.assert_array_equal(img[p.Y, p.X], want)
    assert (img[p.owner < 0] == (9, 8, 7)).all()
    print(f"{F} faces, {p.C} charts, rho {p.rho:.3f}, {p.total} texels ({p.total / Rr ** 2:.1%}), overlap {p.overlap}")


@pytest.mark.parametrize("get,Rr,g", [(soup, 64, 2), (T.sphere_mesh, 512, 2)], ids=["hand_soup", "sphere"])
def test_second_run_is_identical_and_ranges_split(get, Rr, g):
    v, f, n = get()
    a, b = proj_run(v, f, n, Rr, g), proj_run(v, f, n, Rr, g)
    for k in ("face_class", "face_chart", "extents", "rects", "uvs", "owner_ab", "owner", "x", "d"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["rho"], a["total"], a["overlap"]) == (b["rho"], b["total"], b["overlap"])
    p = plan_of(get, Rr, g)
    chart_of = p.face_chart[p.owner[p.Y, p.X]]
    cut = int(np.nonzero(chart_of != chart_of[0])[0][0])                           # the first texel of another chart
    t0, t1 = max(0, cut - 37), min(p.total, cut + 91)
    part = proj_run(v, f, n, Rr, g, t0=t0, t1=t1)
    assert len({int(c) for c in chart_of[t0:t1]}) >= 2
    for k in ("x", "d"):
        assert part[k][:t1 - t0].tobytes() == a[k][t0:t1].tobytes(), k
        assert (part[k][t1 - t0:] == PAD).all()
    img = part["image"]
    inside = np.zeros(p.total, bool)
    inside[t0:t1] = True
    assert (img[p.Y[~inside], p.X[~inside]] == 77).all()                           # the store wrote its range only
    want = np.rint(np.clip(part["rgb"][:t1 - t0], 0, 1) * f32(255)).astype(np.uint8)
    np.testing.assert_array_equal(img[p.Y[inside], p.X[inside]], want)


def test_capacities_and_bad_index():
    from customnerf_amd import mesh
    v, f, n = decimated_sphere()
    F, Rr = len(f), 256
    p = plan_of(decimated_sphere, Rr, 2)
    got = proj_run(v, f, n, Rr, 2, max_faces=F - 5, max_points=1000)
    for k in ("face_class", "face_chart", "uvs"):
        assert (got[k][F - 5:] == PAD).all(), k
    np.testing.assert_array_equal(got["face_chart"][:F - 5], p.face_chart[:F - 5])
    np.testing.assert_array_equal(bits(got["uvs"][:F - 5]), bits(p.uvs[:F - 5]))
    np.testing.assert_array_equal(got["owner"], p.owner)
    few = proj_run(v, f, n, Rr, 2, max_charts=p.C - 2, pack=False)               # the charts beyond the capacity are not reported
    assert few["C"] == p.C and (few["extents"][p.C - 2:] == PAD).all()
    np.testing.assert_array_equal(bits(few["extents"][:p.C - 2]), bits(p.extents[:p.C - 2]))
    xr, _ = P.points(p, v, f, n, 0, 1000)
    np.testing.assert_array_equal(bits(got["x"][:1000]), bits(xr))
    assert (got["x"][1000:] == PAD).all() and (got["d"][1000:] == PAD).all()
    for bad in (len(v), -1):
        fb = f.copy()
        fb[F // 2, 1] = bad
        got = proj_run(v, fb, n, Rr, 2, pack=False)
        assert got["flags"] == 1 and got["C"] == 0 and got["total"] == 0
        for k in ("face_class", "face_chart", "extents", "uvs", "owner_ab", "owner", "x", "d"):
            assert (got[k] == PAD).all(), k
        assert (got["image"] == 77).all()
        with pytest.raises(ValueError, match="outside"):
            mesh.bake_texture(cuda(v), cuda(fb), Rr, lambda x, d: x, layout='projected')
        with pytest.raises(ValueError, match="outside"):
            mesh.chart_plan(cuda(v), cuda(fb), Rr)


def test_chart_plan_members():
    from customnerf_amd import mesh
    v, f, n = decimated_sphere()
    p = plan_of(decimated_sphere, 256, 2)
    cp = mesh.chart_plan(cuda(v), cuda(f), 256, normals=cuda(n))
    assert (cp.resolution, cp.gutter, cp.charts, cp.density, cp.texels, cp.overlap_texels) == (256, 2, p.C, p.rho, p.total, p.overlap)
    assert cp.coverage == p.total / 256 ** 2
    np.testing.assert_array_equal(cp.rects.cpu().numpy(), p.rects)
    np.testing.assert_array_equal(cp.face_chart.cpu().numpy(), p.face_chart)
    np.testing.assert_array_equal(cp.face_class.cpu().numpy(), p.classes)
    np.testing.assert_array_equal(cp.owner.cpu().numpy(), p.owner)
    p0 = P.plan(v, f, 100, None, 0)                                                # no normals, no gutter, a resolution that is no power of two
    c0 = mesh.chart_plan(cuda(v), cuda(f), 100, gutter=0)
    assert (c0.charts, c0.density, c0.texels) == (p0.C, p0.rho, p0.total)
    np.testing.assert_array_equal(c0.owner.cpu().numpy(), p0.owner)


@pytest.mark.parametrize("get,Rr", [(T.cube, 64), (T.quad, 512)], ids=["cube", "quad"])
def test_affine_colour_bake(tmp_path, get, Rr):
    """colour = 0.5 + 0.4 x baked on meshes whose charts are planar, written (OBJ + PNG), read back: bilinear lookup at random points of every
    UV triangle gives the colour of the surface point within the uint8 rounding"""
    from customnerf_amd import mesh
    v, f, _ = get()
    p = plan_of(get, Rr, 2)
    uvs, tex = mesh.bake_texture(cuda(v), cuda(f), Rr, lambda x, d: 0.5 + 0.4 * x, chunk=10_000, layout='projected')
    path = str(tmp_path / "affine.obj")
    mesh.write_obj(path, v, f, uvs=uvs, texture=tex)
    o = A.read_obj(path)
    img = A.read_png(str(tmp_path / "affine.png"))
    np.testing.assert_array_equal(img, tex.cpu().numpy())
    assert np.array_equal(o["verts"], v) and np.array_equal(o["f"][..., 0] - 1, f)
    np.testing.assert_array_equal(bits(uvs.cpu().numpy()), bits(p.uvs))
    uv = o["uvs"][o["f"][..., 1] - 1].astype(np.float64)
    np.testing.assert_array_equal(o["uvs"].reshape(-1, 3, 2), p.uvs)
    rng = np.random.default_rng(0)
    w = np.concatenate([np.eye(3), [[0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]], rng.dirichlet((1, 1, 1), 40)])
    pts_uv = np.einsum("kc,fcd->fkd", w, uv).reshape(-1, 2)
    pts = np.einsum("kc,fcd->fkd", w, v[f].astype(np.float64)).reshape(-1, 3)
    got = A.bilinear(img, pts_uv[:, 0], pts_uv[:, 1]) / 255.0
    err = np.abs(got - (0.5 + 0.4 * pts))
    print(f"{p.C} charts: worst colour error {err.max() * 255:.4f} levels (bound 0.6)")
    assert err.max() <= 0.6 / 255, err.max()
    flipped = A.bilinear(img, pts_uv[:, 0], 1.0 - pts_uv[:, 1]) / 255.0            # a v-flipped lookup would not pass
    assert np.abs(flipped - (0.5 + 0.4 * pts)).max() > 10 / 255


@pytest.mark.parametrize("get,Rr", [(decimated_sphere, 256), (T.torus_mesh, 1024)], ids=["decimated_sphere", "torus"])
def test_curved_texture_is_the_restatements(get, Rr):
    """on a curved mesh neighbouring texels lie on different planes, so no colour bound holds: the texture is the restatement's, bit for bit"""
    from customnerf_amd import mesh
    v, f, n = get()
    p = plan_of(get, Rr, 2)
    uvs, tex = mesh.bake_texture(cuda(v), cuda(f), Rr, lambda x, d: 0.5 + 0.4 * x, normals=cuda(n), chunk=50_000, fill=(3, 2, 1),
                                 layout='projected')
    xr, _ = P.points(p, v, f, n)
    want = np.full((Rr, Rr, 3), (3, 2, 1), np.uint8)
    want[p.Y, p.X] = np.rint(np.clip(f32(0.5) + f32(0.4) * xr, 0, 1) * f32(255)).astype(np.uint8)
    np.testing.assert_array_equal(tex.cpu().numpy(), want)
    np.testing.assert_array_equal(bits(uvs.cpu().numpy()), bits(p.uvs))


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_store_matches_field(dtype_guard, fp16):
    from customnerf_amd import mesh
    model = gaussian_model(dtype_guard, fp16)
    m = model.extract_mesh(resolution=40, threshold=10.0, aabb=AABB)
    v, f, n = m['verts'], m['faces'], m['normals']
    Rr = 256
    vh, fh, nh = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    p = P.plan(vh, fh, Rr, nh, 2)
    seen = []

    def color_fn(x, d):
        rgbc = model(x, d)[1]
        seen.append((x.clone(), d.clone(), rgbc.clone()))
        return rgbc                                                                # [N, 4]: the first three are used

    fill = (1, 2, 3)
    uvs, tex = mesh.bake_texture(v, f, Rr, color_fn, normals=n, chunk=20_000, fill=fill, layout='projected')
    total = p.total
    assert sum(len(a[0]) for a in seen) == total and len(seen) == -(-total // 20_000)
    x = torch.cat([a[0] for a in seen]).cpu().numpy()
    d = torch.cat([a[1] for a in seen]).cpu().numpy()
    rgb = torch.cat([a[2] for a in seen])[:, :3].float().clamp(0, 1)
    want = (rgb * 255).round().to(torch.uint8).cpu().numpy()
    xr, dr = P.points(p, vh, fh, nh)
    np.testing.assert_array_equal(bits(x), bits(xr))
    np.testing.assert_allclose(d, dr, rtol=0, atol=2e-6)
    t = tex.cpu().numpy()
    np.testing.assert_array_equal(t[p.Y, p.X], want)                               # every owned texel: the rounded colour
    assert (t[p.owner < 0] == fill).all()                                          # every other texel: the fill
    np.testing.assert_array_equal(bits(uvs.cpu().numpy()), bits(p.uvs))


def test_source_and_normal_map():
    from customnerf_amd import mesh
    v, f, n = decimated_sphere()
    sv, sf, sn = T.sphere_mesh()
    p = plan_of(decimated_sphere, 256, 2)
    src = mesh.bake_source(cuda(sv), cuda(sf), cuda(sn))
    uvs, tex, extra = mesh.bake_texture(cuda(v), cuda(f), 256, lambda x, d: 0.5 + 0.4 * x, normals=cuda(n), chunk=30_000, layout='projected',
                                        source=src, normal_map=True)
    assert int(extra['kinds'].sum()) == p.total
    nm = extra['normal_map'].cpu().numpy()
    assert nm.shape == (256, 256, 3) and (nm[p.owner < 0] == 128).all()
    own = nm[p.Y, p.X].astype(np.float64) / 255.0 * 2.0 - 1.0                      # unit normals of the source, through the uint8 rounding
    assert np.abs(np.linalg.norm(own, axis=1) - 1.0).max() < 0.02
    np.testing.assert_array_equal(bits(uvs.cpu().numpy()), bits(p.uvs))
    t = tex.cpu().numpy()
    assert (t[p.owner < 0] == 0).all()
    r = np.linalg.norm((t[p.Y, p.X].astype(np.float64) / 255.0 - 0.5) / 0.4, axis=1)     # a projected point lies on the source sphere
    missed = int(extra['kinds'][0]) / p.total                                      # 0.012: sqrt(3) half a level / 0.4, and the lattice's error
    assert (np.abs(r - 0.9) < 0.012).mean() >= 1.0 - missed - 0.01, ((np.abs(r - 0.9) < 0.012).mean(), missed)
    _, tex2, extra2 = mesh.bake_texture(cuda(v), cuda(f), 256, lambda x, d: 0.5 + 0.4 * x, normals=cuda(n), layout='projected', normal_map=True)
    assert extra2['kinds'].cpu().tolist() == [0, 0, 0, 0] and (extra2['normal_map'].cpu().numpy()[p.owner < 0] == 128).all()


def test_save_mesh_projected_layout_and_render(dtype_guard, tmp_path):
    from customnerf_amd import scene
    model = gaussian_model(dtype_guard, False)
    kw = dict(resolution=96, threshold=10.0, aabb=AABB, keep_largest=True, target_faces=1000)
    mo = model.save_mesh(str(tmp_path / "blob.obj"), texture=256, texture_layout='projected', **kw)
    assert mo['texture_layout'] == 'projected'
    o = A.read_obj(str(tmp_path / "blob.obj"))
    assert o["mtllib"] == "blob.mtl" and "map_Kd blob.png" in open(str(tmp_path / "blob.mtl")).read()
    img = A.read_png(str(tmp_path / "blob.png"))
    assert img.shape == (256, 256, 3)
    np.testing.assert_array_equal(img, mo['texture'].cpu().numpy())
    v, f, n = mo['verts'].cpu().numpy(), mo['faces'].cpu().numpy(), mo['normals'].cpu().numpy()
    assert np.array_equal(o["verts"], v) and np.array_equal(o["f"][..., 0] - 1, f) and len(f) in (999, 1000)
    p = P.plan(v, f, 256, n, 2)
    uv = mo['uvs'].cpu().numpy()
    np.testing.assert_array_equal(bits(uv), bits(p.uvs))
    np.testing.assert_array_equal(o["uvs"].reshape(-1, 3, 2), uv)
    assert (img[p.owner < 0] == 0).all() and (img[p.owner >= 0].max(axis=1) > 0).mean() > 0.99
    print(f"{len(f)} faces, {p.C} charts, coverage {p.total / 256 ** 2:.1%}, overlap {p.overlap}")
    # the preview of the export is the shade restatement's, fed the same uvs and texture
    H = W = 128
    pose, intr = scene.camera_pose(3, radius=1.2), scene.intrinsics(H, W)
    image, mask, _ = model.render_mesh(mo, pose, intr, H, W)
    vis = RS.visibility(v, f, pose, intr, H, W)
    want, wmask = RS.shade(vis, v, f, 'texture', uvs=uv, texture=img)
    got = image.cpu().numpy()
    assert (wmask > 0).sum() > 1000
    np.testing.assert_array_equal(mask.cpu().numpy(), wmask > 0)
    np.testing.assert_array_equal(got, want)
    assert model.extract_mesh(resolution=24, threshold=10.0, aabb=AABB)['texture_layout'] == 'uniform'      # the default is what it was


def test_value_errors():
    from customnerf_amd import mesh
    v, f, n = (cuda(a) for a in T.sphere_mesh())
    fn = lambda x, d: x                                                            # noqa: E731
    for g in (9, -1):
        with pytest.raises(ValueError, match="gutter"):
            mesh.bake_texture(v, f, 512, fn, layout='projected', gutter=g)
        with pytest.raises(ValueError, match="gutter"):
            mesh.chart_plan(v, f, 512, gutter=g)
    with pytest.raises(ValueError, match="gutter"):
        mesh.bake_texture(v, f, 512, fn, layout='uniform', gutter=2)
    with pytest.raises(ValueError, match="gutter"):
        mesh.bake_texture(v, f, 512, fn, gutter=2)
    with pytest.raises(ValueError, match="resolution"):
        mesh.bake_texture(v, f, 8, fn, layout='projected')
    with pytest.raises(ValueError, match="resolution"):
        mesh.chart_plan(v, f, 8)
    sv, sf, sn, _ = T.hand_soup()                                                  # six charts of 17 x 17 texels at least: 16 x 16 holds none
    with pytest.raises(ValueError, match="decimate the mesh"):
        mesh.bake_texture(cuda(sv), cuda(sf), 16, fn, layout='projected', gutter=8)
    with pytest.raises(ValueError, match="decimate the mesh"):
        mesh.chart_plan(cuda(sv), cuda(sf), 16, gutter=3)                          # 2 x 2 cells of 7 x 7 texels hold 4
    assert mesh.chart_plan(cuda(sv), cuda(sf), 16, normals=cuda(sn), gutter=1).charts == 6
    with pytest.raises(ValueError, match="layout") as e:
        mesh.bake_texture(v, f, 512, fn, layout='charts')
    assert all(name in str(e.value) for name in ("'uniform'", "'area'", "'projected'"))
