"""GPU: the mesh rasteriser (csrc/mesh_raster.hip) against its NumPy restatement (tests/raster_restatement.py) — face, depth and barycentrics
bit-equal over hand-made, marching-cubes and decimation meshes and a view-filling quad, under both camera conventions; culling, near drops;
the four shading modes; a baked affine colour seen through render_mesh; and end to end through NeRFRenderer.render_mesh."""
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
import raster_restatement as RS  # noqa: E402
from mesh_testlib import AABB, R_SPHERE, cuda, decimate_meshes, dtype_guard, gaussian_model, lattice  # noqa: E402,F401

SENTINEL = -7.0
PAD = 8


def sphere_mesh(n=40, r=0.9):
    (X, Y, Z), sp = lattice((n, n, n), -1.0, 1.0)
    return R.marching_cubes((r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))


def torus_mesh():
    (X, Y, Z), sp = lattice((48, 44, 36), -1.0, 1.0)
    q = np.sqrt(X ** 2 + Y ** 2) - 0.6
    return R.marching_cubes((0.25 - np.sqrt(q ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))


def unit_ball(v):
    """the vertices moved and scaled into the unit ball, float32"""
    v = np.asarray(v, np.float64)
    c = 0.5 * (v.min(0) + v.max(0))
    return ((v - c) / np.linalg.norm(v - c, axis=1).max()).astype(np.float32)


def view_quad(c2w, opencv, half=5.0):
    """two triangles facing the camera in the plane through the point it looks at (the origin), far larger than the view"""
    m = c2w.astype(np.float64)
    fwd = m[:, 2] if opencv else -m[:, 2]
    o = m[:, 3] + np.linalg.norm(m[:, 3]) * fwd
    v = np.array([o + half * (sx * m[:, 0] + sy * m[:, 1]) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def parity_meshes():
    rng = np.random.default_rng(9)
    v = rng.standard_normal((30, 3)).astype(np.float32)
    f = rng.permutation(30).reshape(10, 3).astype(np.int32)
    yield "soup", v, np.concatenate([f, [[0, 0, 1], [2, 2, 2], [0, 1, 2]]]).astype(np.int32)       # with zero-area faces
    sv, sf, _ = sphere_mesh()
    yield "sphere", sv, sf
    tv, tf, _ = torus_mesh()
    yield "torus", tv, tf
    for name, dv, df, _ in decimate_meshes():
        yield name, unit_ball(dv), df


MESHES = list(parity_meshes())
# (convention, view, elevation, radius, H, W): two poses per convention; a non-square size and widths that are no multiple of 64
CAMERAS = [("nerfstudio", 3, 20.0, 3.5, 128, 128), ("nerfstudio", 6, -40.0, 2.2, 75, 100), ("ngp", 1, 35.0, 3.0, 96, 130), ("ngp", 5, 5.0, 1.6, 61, 47)]


def camera(convention, view, elev, radius, H, W):
    from customnerf_amd import scene
    return scene.camera_pose(view, radius=radius, elev_deg=elev, opencv=convention == "ngp"), scene.intrinsics(H, W)


def gpu_visibility(v, f, c2w, intr, H, W, convention="nerfstudio", near=0.01, cull="none"):
    """cnerf_mesh_raster_visibility into sentinel-padded buffers -> (face, depth, bary, counts) arrays with their padding"""
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib, check, ptr, stream
    gv, gf = cuda(np.asarray(v, np.float32)), cuda(np.asarray(f, np.int32))
    V, F = gv.shape[0], gf.shape[0]
    nbytes = mesh.raster_workspace_bytes(V, F, H, W)
    ws = torch.full((nbytes + 256,), 0x5a, dtype=torch.uint8, device="cuda")
    face = torch.full((H * W + PAD,), int(SENTINEL), dtype=torch.int32, device="cuda")
    depth = torch.full((H * W + PAD,), SENTINEL, device="cuda")
    bary = torch.full((3 * H * W + PAD,), SENTINEL, device="cuda")
    counts = torch.full((2 + PAD,), 0x55, dtype=torch.int32, device="cuda")
    m = (C.c_float * 12)(*np.asarray(c2w, np.float32)[:3].ravel().tolist())
    check(lib.cnerf_mesh_raster_visibility(ptr(gv) if V else None, V, ptr(gf) if F else None, F, m, *intr, H, W, RS.CONVENTIONS[convention],
                                           near, RS.CULL[cull], ptr(ws), nbytes, ptr(face), ptr(depth), ptr(bary), ptr(counts), stream()), "vis")
    assert (ws[nbytes:] == 0x5a).all()
    return tuple(t.cpu().numpy() for t in (face, depth, bary, counts))


def assert_same_visibility(got, want, H, W):
    face, depth, bary, counts = got
    n = H * W
    assert (face[n:] == int(SENTINEL)).all() and (depth[n:] == SENTINEL).all() and (bary[3 * n:] == SENTINEL).all() and (counts[2:] == 0x55).all()
    assert counts[1] == (1 if want['bad'] else 0) and counts[0] == want['dropped']
    np.testing.assert_array_equal(face[:n].reshape(H, W), want['face'])
    np.testing.assert_array_equal(depth[:n].reshape(H, W).view(np.uint32), want['depth'].view(np.uint32))
    np.testing.assert_array_equal(bary[:3 * n].reshape(H, W, 3).view(np.uint32), want['bary'].view(np.uint32))


@pytest.mark.parametrize("cam", CAMERAS, ids=[f"{c[0]}{c[1]}_{c[4]}x{c[5]}" for c in CAMERAS])
@pytest.mark.parametrize("name,v,f", MESHES, ids=[m[0] for m in MESHES])
def test_visibility_matches_restatement(name, v, f, cam):
    """face equal, depth and bary bit-equal, the dropped count equal, a second run bit-identical, the padding untouched"""
    convention, H, W = cam[0], cam[4], cam[5]
    c2w, intr = camera(*cam)
    want = RS.visibility(v, f, c2w, intr, H, W, convention=convention)
    runs = [gpu_visibility(v, f, c2w, intr, H, W, convention=convention) for _ in range(2)]
    assert_same_visibility(runs[0], want, H, W)
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    print(f"{name}: {int((want['face'] >= 0).sum())} of {H * W} pixels hit, {want['dropped']} faces dropped")
    if name != "soup":
        assert (want['face'] >= 0).sum() > 50


@pytest.mark.parametrize("cam", CAMERAS + [("nerfstudio", 2, 30.0, 3.0, 200, 333)], ids=lambda c: f"{c[0]}{c[1]}_{c[4]}x{c[5]}")
def test_view_filling_quad(cam):
    """two faces whose boxes are the whole image: the large-face path, every pixel hit"""
    convention, H, W = cam[0], cam[4], cam[5]
    c2w, intr = camera(*cam)
    v, f = view_quad(c2w, convention == "ngp")
    want = RS.visibility(v, f, c2w, intr, H, W, convention=convention)
    assert (want['face'] >= 0).all() and want['dropped'] == 0 and set(np.unique(want['face'])) == {0, 1}
    got = gpu_visibility(v, f, c2w, intr, H, W, convention=convention)
    assert_same_visibility(got, want, H, W)
    # mixed with small faces in front of it and behind it
    sv, sf, _ = sphere_mesh(24, 0.5)
    v2, f2 = np.concatenate([sv, v]), np.concatenate([sf, f + len(sv)]).astype(np.int32)
    want = RS.visibility(v2, f2, c2w, intr, H, W, convention=convention)
    assert_same_visibility(gpu_visibility(v2, f2, c2w, intr, H, W, convention=convention), want, H, W)
    assert (want['face'] >= 0).all() and (want['face'] < len(sf)).sum() > 20 and (want['face'] >= len(sf)).sum() > 20


@pytest.mark.parametrize("cull", ["none", "back", "front"])
def test_cull_near_and_dropped(cull):
    from customnerf_amd import mesh, scene
    v, f, _ = sphere_mesh()
    H, W = 90, 120
    # from outside
    c2w, intr = scene.camera_pose(5, radius=2.5), scene.intrinsics(H, W)
    want = RS.visibility(v, f, c2w, intr, H, W, cull=cull)
    assert_same_visibility(gpu_visibility(v, f, c2w, intr, H, W, cull=cull), want, H, W)
    # from inside: part of the sphere lies behind the camera and is dropped; what remains equals the restatement
    c2w = scene.camera_pose(0, radius=0.5, elev_deg=10)
    want = RS.visibility(v, f, c2w, intr, H, W, cull=cull)
    assert 0 < want['dropped'] < len(f)
    assert_same_visibility(gpu_visibility(v, f, c2w, intr, H, W, cull=cull), want, H, W)
    vis = mesh.rasterize(cuda(v), cuda(f), c2w, intr, H, W, cull=cull)
    assert vis['dropped'] == want['dropped'] and np.array_equal(vis['face'].cpu().numpy(), want['face'])
    hit = want['face'] >= 0
    if cull == "back":
        assert not hit.any()                                                    # the inside of an outward-wound wall is back-facing
    else:
        assert hit.sum() > 1000                                                 # cull='front' sees the far wall
    # a larger near drops more
    far = RS.visibility(v, f, c2w, intr, H, W, cull=cull, near=0.8)
    assert far['dropped'] > want['dropped']
    assert_same_visibility(gpu_visibility(v, f, c2w, intr, H, W, cull=cull, near=0.8), far, H, W)
    # c2w as a [4, 4] tensor
    m44 = torch.eye(4)
    m44[:3] = torch.from_numpy(c2w)
    vis = mesh.rasterize(cuda(v), cuda(f), m44.cuda(), intr, H, W, cull=cull)
    assert np.array_equal(vis['face'].cpu().numpy(), want['face'])


def gpu_shade(vis, v, f, mode, H, W, colors=None, uvs=None, texture=None, normals=None, depth_range=(0.0, 1.0), bg=(0, 0, 0)):
    from customnerf_amd._lib import lib, check, ptr, stream
    g = {k: cuda(a) for k, a in dict(face=vis['face'], depth=vis['depth'], bary=vis['bary'], v=np.asarray(v, np.float32), f=np.asarray(f, np.int32),
                                     colors=colors, uvs=uvs, texture=texture, normals=normals).items()}
    image = torch.full((3 * H * W + PAD,), 77, dtype=torch.uint8, device="cuda")
    mask = torch.full((H * W + PAD,), 77, dtype=torch.uint8, device="cuda")
    p = lambda k: None if g[k] is None else ptr(g[k])                           # noqa: E731
    check(lib.cnerf_mesh_raster_shade(p("face"), p("depth"), p("bary"), H, W, p("f"), len(v), len(f), ("colors", "texture", "normals", "depth").index(mode),
                                      p("colors"), p("uvs"), p("texture"), 0 if texture is None else texture.shape[0], p("v"), p("normals"),
                                      depth_range[0], depth_range[1], (C.c_uint8 * 3)(*bg), ptr(image), ptr(mask), stream()), "shade")
    image, mask = image.cpu().numpy(), mask.cpu().numpy()
    assert (image[3 * H * W:] == 77).all() and (mask[H * W:] == 77).all()
    return image[:3 * H * W].reshape(H, W, 3), mask[:H * W].reshape(H, W)


@pytest.mark.parametrize("cam", [CAMERAS[0], CAMERAS[2]], ids=lambda c: c[0])
def test_shading_matches_restatement(cam):
    """every mode within one level of the restatement's image, the mask equal"""
    convention, H, W = cam[0], cam[4], cam[5]
    c2w, intr = camera(*cam)
    v, f, n = torus_mesh()
    rng = np.random.default_rng(5)
    n = n.copy()
    n[rng.integers(0, len(n), 200)] = 0                                         # vanishing normals: the face normal steps in
    vis = RS.visibility(v, f, c2w, intr, H, W, convention=convention)
    hit = vis['face'] >= 0
    assert hit.sum() > 500
    colors = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    uvs = rng.uniform(-0.2, 1.2, (len(f), 3, 2)).astype(np.float32)             # beyond [0, 1]: clamped to the edge
    tex = rng.integers(0, 256, (37, 37, 3)).astype(np.uint8)
    d0, d1 = float(vis['depth'][hit].min()), float(vis['depth'][hit].max())
    for mode, kw in (("colors", dict(colors=colors)), ("texture", dict(uvs=uvs, texture=tex)), ("normals", dict(normals=n)),
                     ("depth", dict(depth_range=(d0, d1))), ("depth", dict(depth_range=(d1, d1)))):
        bg = (9, 80, 200)
        want, wmask = RS.shade(vis, v, f, mode, bg=bg, **kw)
        got, mask = gpu_shade(vis, v, f, mode, H, W, bg=bg, **kw)
        np.testing.assert_array_equal(mask, wmask)
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        print(f"{mode}: {int((diff > 0).sum())} of {diff.size} values differ, worst {int(diff.max())}")
        assert diff.max() <= 1
        assert (got[~hit] == bg).all()


def test_render_mesh_modes_and_defaults():
    from customnerf_amd import mesh, scene
    v, f, n = sphere_mesh(24)
    gv, gf, gn = cuda(v), cuda(f), cuda(n)
    H, W = 72, 96
    c2w, intr = scene.camera_pose(3), scene.intrinsics(H, W)
    vis = RS.visibility(v, f, c2w, intr, H, W)
    hit = vis['face'] >= 0
    # default shading without colours or texture: normals, computed from the mesh when none are given
    image, mask, gvis = mesh.render_mesh(gv, gf, c2w, intr, H, W, bg=(5, 6, 7))
    assert image.dtype == torch.uint8 and tuple(image.shape) == (H, W, 3) and mask.dtype == torch.bool and tuple(mask.shape) == (H, W)
    assert np.array_equal(mask.cpu().numpy(), hit) and np.array_equal(gvis['face'].cpu().numpy(), vis['face']) and gvis['dropped'] == 0
    vn = mesh.vertex_normals(gv, gf).cpu().numpy()
    want, _ = RS.shade(vis, v, f, 'normals', normals=vn, bg=(5, 6, 7))
    assert np.abs(image.cpu().numpy().astype(np.int32) - want).max() <= 1
    # colours are picked when given; depth defaults to the range of the hit depths
    colors = np.clip(np.rint((0.5 + 0.4 * v) * 255), 0, 255).astype(np.uint8)
    image, _, _ = mesh.render_mesh(gv, gf, c2w, intr, H, W, colors=cuda(colors), normals=gn)
    want, _ = RS.shade(vis, v, f, 'colors', colors=colors)
    assert np.abs(image.cpu().numpy().astype(np.int32) - want).max() <= 1
    image, _, _ = mesh.render_mesh(gv, gf, c2w, intr, H, W, shading='depth')
    want, _ = RS.shade(vis, v, f, 'depth', depth_range=(vis['depth'][hit].min(), vis['depth'][hit].max()))
    assert np.abs(image.cpu().numpy().astype(np.int32) - want).max() <= 1
    assert image.cpu().numpy()[hit].min() == 0 and image.cpu().numpy()[hit].max() == 255
    # inconsistent arguments
    for kw in (dict(shading='colors'), dict(shading='texture'), dict(shading='phong'), dict(colors=cuda(colors[:-1])), dict(bg=(0, 0, 256)),
               dict(colors=cuda(colors).float()), dict(shading='texture', uvs=torch.zeros(3, 3, 2, device="cuda"), texture=cuda(colors)),
               dict(shading='depth', depth_range=(0.0, float("inf"))), dict(convention='opengl'), dict(cull='both'), dict(near=float("nan"))):
        with pytest.raises(ValueError, match="render_mesh|rasterize"):
            mesh.render_mesh(gv, gf, c2w, intr, H, W, **kw)
    with pytest.raises(ValueError, match="rasterize"):
        mesh.rasterize(gv, gf, c2w[:2], intr, H, W)
    with pytest.raises(ValueError, match="rasterize"):
        mesh.rasterize(gv, gf, c2w, (0.0, 1.0, 2.0, 3.0), H, W)
    with pytest.raises(ValueError, match="rasterize"):
        mesh.rasterize(gv, gf, c2w, intr, 1 << 16, 1 << 15)


def test_baked_affine_colour_through_render_mesh():
    """colour = 0.5 + 0.4 x baked into the atlas and rendered: every hit pixel shows the colour of its surface point p = sum beta_k v_k (the
    restatement's barycentrics) within (0.6 + 0.5) / 255 — 0.6 / 255 for a bilinear lookup inside a UV triangle (test_affine_colour_bake),
    0.5 / 255 for the output rounding — plus 1e-4 of float slack.  A v-flipped lookup or affine (not perspective-correct) barycentrics must
    not pass the same check."""
    from customnerf_amd import mesh, scene
    v, f, n = sphere_mesh()
    gv, gf = cuda(v), cuda(f)
    Rr = 6 * A.layout(len(f), 16384)[0]
    uvs, tex = mesh.bake_texture(gv, gf, Rr, lambda x, d: 0.5 + 0.4 * x, normals=cuda(n), chunk=100_000)
    H = W = 128
    c2w, intr = scene.camera_pose(3, radius=1.5), scene.intrinsics(H, W)         # close: perspective matters across the sphere
    vis = RS.visibility(v, f, c2w, intr, H, W)
    hit = vis['face'] >= 0
    image, mask, gvis = mesh.render_mesh(gv, gf, c2w, intr, H, W, uvs=uvs, texture=tex)
    assert np.array_equal(mask.cpu().numpy(), hit)
    np.testing.assert_array_equal(gvis['bary'].cpu().numpy().view(np.uint32), vis['bary'].view(np.uint32))
    tri = v[f[vis['face'][hit]]].astype(np.float64)
    p = (vis['bary'][hit].astype(np.float64)[..., None] * tri).sum(1)
    tol = (0.6 + 0.5) / 255 + 1e-4
    err = np.abs(image.cpu().numpy()[hit] / 255.0 - (0.5 + 0.4 * p)).max()
    print(f"worst colour error {err * 255:.3f} levels (bound {tol * 255:.3f})")
    assert err <= tol
    # teeth: the same check on a v-flipped lookup and on affine barycentrics
    uv_h, tex_h = uvs.cpu().numpy(), tex.cpu().numpy()
    flipped = uv_h.copy()
    flipped[..., 1] = 1.0 - flipped[..., 1]
    img_flip, _ = RS.shade(vis, v, f, 'texture', uvs=flipped, texture=tex_h)
    _, _, _, _, z = RS.project(v, c2w, intr)
    aff = vis['bary'].astype(np.float64).copy()
    aff[hit] *= z[f[vis['face'][hit]]]                                            # beta_k z_k / depth = b_k, the screen-space weights
    aff[hit] /= aff[hit].sum(-1, keepdims=True)
    img_aff, _ = RS.shade(dict(vis, bary=aff.astype(np.float32)), v, f, 'texture', uvs=uv_h, texture=tex_h)
    e_flip = np.abs(img_flip[hit] / 255.0 - (0.5 + 0.4 * p)).max()
    e_aff = np.abs(img_aff[hit] / 255.0 - (0.5 + 0.4 * p)).max()
    print(f"v-flipped {e_flip * 255:.2f} levels, affine barycentrics {e_aff * 255:.2f} levels")
    assert e_flip > tol or e_aff > tol


def analytic_sphere(c2w, intr, H, W, r):
    """'nerfstudio' rays through the pixel centres against the sphere |x| = r: (distance of the ray from the centre, camera-axis depth of
    the first hit (NaN on a miss)), [H, W] each"""
    fx, fy, cx, cy = intr
    iy, ix = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cam = np.stack([(ix + 0.5 - cx) / fx, -(iy + 0.5 - cy) / fy, -np.ones_like(ix, float)], -1)
    ln = np.linalg.norm(cam, axis=-1)
    m = np.asarray(c2w, np.float64)
    o, d = m[:, 3], (cam @ m[:, :3].T) / ln[..., None]
    od = (d * o).sum(-1)
    dist = np.linalg.norm(o - od[..., None] * d, axis=-1)
    with np.errstate(invalid="ignore"):
        return dist, (-od - np.sqrt(r * r - dist * dist)) / ln


def test_renderer_render_mesh(dtype_guard, tmp_path):
    """NeRFRenderer.render_mesh on a decimated, textured export of a Gaussian blob: the PNG is the returned image; hit depths outside the
    one-lattice-step silhouette band (at most 8 % of the image) are within one lattice step of the analytic sphere (measured on an MI355X:
    band 2.8 % of the image, worst depth error 0.0043 against a step of 0.0105).
    The vertex-colour render of the PLY-path mesh and the texture render are compared and the agreement is printed, not asserted: the
    proposed figure (within 2 levels on 99 % of the common hit pixels) does not hold, and is not loosened to fit.  Measured: within 2
    levels on 73.65 % of the 2664 common hit pixels, worst difference 8 levels.  Both renders hit the same pixels and agree at the vertices
    (the corner-texel check of test_save_mesh_textured_obj); between them the vertex colours are interpolated linearly over faces that
    span about 9 degrees of this 1000-face sphere, while the texture holds the field's colour at about 40 texels per face, and the field's
    colour here is a nonlinear function of the viewing direction -normal.  The test also prints each render against the field evaluated at
    every pixel's own surface point, which bears this out: the texture render is within 1 level of the field on every pixel (worst 0.94),
    the vertex-colour render within 2 levels on 60.3 % (worst 8.2)."""
    from customnerf_amd import scene
    model = gaussian_model(dtype_guard, False)
    kw = dict(resolution=96, threshold=10.0, aabb=AABB, keep_largest=True, target_faces=1000)
    m = model.extract_mesh(texture=256, **kw)
    H = W = 128
    pose, intr = scene.camera_pose(3, radius=1.2), scene.intrinsics(H, W)
    path = str(tmp_path / "preview.png")
    image, mask, vis = model.render_mesh(m, pose, intr, H, W, path=path)
    img = image.cpu().numpy()
    np.testing.assert_array_equal(A.read_png(path), img)
    hit = mask.cpu().numpy()
    assert np.array_equal(hit, vis['face'].cpu().numpy() >= 0) and vis['dropped'] == 0 and hit.sum() > 1000
    h = 1.0 / 95
    dist, depth = analytic_sphere(pose, intr, H, W, R_SPHERE)
    band = np.abs(dist - R_SPHERE) <= h
    print(f"band share {band.mean():.4f}")
    assert band.mean() <= 0.08
    sel = hit & ~band
    assert (dist[sel] < R_SPHERE).all()                                            # a hit outside the band is a hit of the sphere
    err = np.abs(vis['depth'].cpu().numpy()[sel] - depth[sel]).max()
    print(f"worst depth error {err:.5f} (one lattice step {h:.5f})")
    assert err <= h
    mc = model.extract_mesh(color=True, **kw)                                      # the PLY path's mesh: same geometry, vertex colours
    assert torch.equal(mc['verts'], m['verts']) and torch.equal(mc['faces'], m['faces'])
    image_c, mask_c, _ = model.render_mesh(mc, pose, intr, H, W)
    common = hit & mask_c.cpu().numpy()
    assert common.sum() == hit.sum()
    diff = np.abs(img.astype(np.int32) - image_c.cpu().numpy().astype(np.int32)).max(-1)[common]
    share = (diff <= 2).mean()
    print(f"texture and vertex-colour renders agree within 2 levels on {share:.4f} of {int(common.sum())} pixels, worst {int(diff.max())}")
    # against the field itself at each pixel's surface point, looking along the interpolated normal
    fh, bh = vis['face'].cpu().numpy()[common], vis['bary'].cpu().numpy()[common]
    tri = m['faces'].cpu().numpy()[fh]
    vv, nn = m['verts'].cpu().numpy(), m['normals'].cpu().numpy()
    p = (bh[..., None] * vv[tri]).sum(1)
    d = -(bh[..., None] * nn[tri]).sum(1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    with torch.no_grad():
        rgb = model(cuda(p.astype(np.float32)), cuda(d.astype(np.float32)))[1][:, :3].float().clamp(0, 1).cpu().numpy() * 255
    for nm, im in (("texture", img), ("vertex-colour", image_c.cpu().numpy())):
        e = np.abs(im[common].astype(np.float64) - rgb).max(-1)
        print(f"{nm} render against the field: within 1 level {(e <= 1).mean():.4f}, 2 levels {(e <= 2).mean():.4f}, worst {e.max():.2f}")
    assert (img[~hit] == 0).all() and (img[hit].max(-1) > 0).mean() > 0.99


def test_edge_cases():
    from customnerf_amd import mesh, scene
    from customnerf_amd._lib import lib, ptr, stream
    v, f, _ = sphere_mesh(14)
    gv, gf = cuda(v), cuda(f)
    H, W = 33, 50
    c2w, intr = scene.camera_pose(1), scene.intrinsics(H, W)
    # F = 0: all-empty outputs and an image of bg
    face, depth, bary, counts = gpu_visibility(v, f[:0], c2w, intr, H, W)
    n = H * W
    assert (face[:n] == -1).all() and np.isinf(depth[:n]).all() and (bary[:3 * n] == 0).all() and (counts[:2] == 0).all()
    assert (face[n:] == int(SENTINEL)).all() and (depth[n:] == SENTINEL).all() and (bary[3 * n:] == SENTINEL).all()
    image, mask, vis = mesh.render_mesh(gv, gf[:0], c2w, intr, H, W, bg=(10, 20, 30))
    assert (image.cpu().numpy() == (10, 20, 30)).all() and not mask.any() and vis['dropped'] == 0
    image, mask, _ = mesh.render_mesh(gv[:0], gf[:0], c2w, intr, H, W, shading='depth')
    assert (image.cpu().numpy() == 0).all() and not mask.any()
    # H W = 1, and an empty image
    want = RS.visibility(v, f, c2w, scene.intrinsics(1, 1), 1, 1)
    assert want['face'][0, 0] >= 0
    assert_same_visibility(gpu_visibility(v, f, c2w, scene.intrinsics(1, 1), 1, 1), want, 1, 1)
    vis = mesh.rasterize(gv, gf, c2w, intr, 0, W)
    assert tuple(vis['face'].shape) == (0, W) and tuple(vis['bary'].shape) == (0, W, 3)
    # an index out of range: ValueError, and the C outputs are written as empty
    for badv in (len(v), -1):
        bad = f.copy()
        bad[len(f) // 3, 1] = badv
        with pytest.raises(ValueError, match="outside"):
            mesh.rasterize(gv, cuda(bad), c2w, intr, H, W)
        with pytest.raises(ValueError, match="outside"):
            mesh.render_mesh(gv, cuda(bad), c2w, intr, H, W)
        face, depth, bary, counts = gpu_visibility(v, bad, c2w, intr, H, W)
        assert counts[1] == 1 and (face[:n] == -1).all() and np.isinf(depth[:n]).all() and (bary[:3 * n] == 0).all()
        assert_same_visibility((face, depth, bary, counts), RS.visibility(v, bad, c2w, intr, H, W), H, W)
    # a stale face buffer shades as a miss where it points outside the mesh
    stale = dict(face=np.full((H, W), len(f), np.int32), depth=np.ones((H, W), np.float32), bary=np.full((H, W, 3), 1 / 3, np.float32))
    img, msk = gpu_shade(stale, v, f, 'depth', H, W, bg=(1, 2, 3))
    assert (img == (1, 2, 3)).all() and (msk == 0).all()
    # capacity and argument errors
    nbytes = mesh.raster_workspace_bytes(len(v), len(f), H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = [torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, device="cuda"), torch.empty(3 * n, device="cuda"),
           torch.empty(2, dtype=torch.int32, device="cuda")]
    m = (C.c_float * 12)(*c2w.ravel().tolist())

    def call(ws_bytes=nbytes, fx=intr[0], convention=0, cull=0, counts=out[3]):
        return lib.cnerf_mesh_raster_visibility(ptr(gv), len(v), ptr(gf), len(f), m, fx, intr[1], intr[2], intr[3], H, W, convention, 0.01, cull,
                                                ptr(ws), ws_bytes, ptr(out[0]), ptr(out[1]), ptr(out[2]), None if counts is None else ptr(counts),
                                                stream())
    assert call(ws_bytes=nbytes - 1) == -1 and call(fx=0.0) == -1 and call(convention=2) == -1 and call(cull=3) == -1
    assert call(counts=None) == -2 and call() == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        mesh.render_mesh(gv, gf, c2w, intr, H, W, shading='texture', uvs=torch.zeros(len(f), 3, 2, device="cuda"),
                         texture=torch.zeros(4, 5, 3, dtype=torch.uint8, device="cuda"))
