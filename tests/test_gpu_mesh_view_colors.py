"""GPU: multi-view colour fusion (csrc/mesh_view_colors.hip) against its NumPy restatement (tests/view_colors_restatement.py) — bit-equal
state, counts and resolved colours — the coloured sphere end to end through mesh.rasterize and mesh.ViewColors, and
extract_mesh(color_views=...) / render_view through NeRFNetwork."""
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
import mc_restatement as R  # noqa: E402
import tsdf_restatement as T  # noqa: E402
import view_colors_restatement as V  # noqa: E402
from mesh_testlib import AABB, cuda, dtype_guard, gaussian_model, host  # noqa: E402,F401

BITS = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)             # noqa: E731
SPHERE_BOUND = 1.4e-3                                                            # tests/test_mesh_view_colors_host.py: 2 x the measured 6.6e-4


def view_colors(sc, convention, kind, weights, power, **kw):
    from customnerf_amd import mesh
    return mesh.ViewColors(cuda(sc['images']), cuda(sc['depth']), sc['cams'], V.K, V.TOL, convention=convention, depth_kind=kind,
                           weights=cuda(sc['weights']) if weights else None, power=power, min_cos=V.MIN_COS, near=V.NEAR, **kw)


def device_state(sc, convention, kind, weights, power, cuts=None):
    vc = view_colors(sc, convention, kind, weights, power)
    x, n = cuda(sc['points']), cuda(sc['normals'])
    state = seen = None
    for s in cuts or [None]:
        state, seen = vc.accumulate(x, n, state, seen, views=s)
    return host(state), host(seen).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def restated(n_views, convention, kind, weights, power):
    sc = V.edge_scene(n_views, convention, kind)
    return V.fuse(sc['points'], sc['normals'], sc['images'], sc['depth'], sc['cams'], V.K, V.TOL, convention=convention, depth_kind=kind,
                  weights=sc['weights'] if weights else None, power=power, min_cos=V.MIN_COS, near=V.NEAR)


# ------------------------------------------------------------------------------------------------ 1. accumulate, bit for bit
@pytest.mark.parametrize("n_views", [1, 16, 17, 33])
@pytest.mark.parametrize("kind", ["z", "ray"])
@pytest.mark.parametrize("convention", ["nerfstudio", "ngp"])
def test_accumulate_equals_restatement(convention, kind, n_views):
    """1000 points (not a multiple of 64) laced with the rule's edge cases, views of 40 x 48, one launch, a full one, and 16 + 1 and
    16 + 16 + 1"""
    sc = V.edge_scene(n_views, convention, kind)
    for weights in (True, False):
        for power in (1, 4):
            want, count = restated(n_views, convention, kind, weights, power)
            got, seen = device_state(sc, convention, kind, weights, power)
            assert (count > 0).sum() > (20 if n_views == 1 else 500) and (count == 0).any()
            np.testing.assert_array_equal(seen, count)
            np.testing.assert_array_equal(BITS(got), BITS(want))
            if n_views == 1:                                                     # view 0 decides every laced point as the rule says
                for name, exp in V.EDGE_CASES.items():
                    assert seen[sc['edge'][name]] == (1 if name == 'weight0' and not weights else exp), name


def test_batching_does_not_matter():
    args = ('nerfstudio', 'z', True, 2)
    sc = V.edge_scene(33, 'nerfstudio', 'z')
    once, seen = device_state(sc, *args)
    np.testing.assert_array_equal(BITS(once), BITS(restated(33, *args)[0]))
    for cuts in ([slice(None)], [slice(0, 1), slice(1, 33)], [slice(v, v + 1) for v in range(33)], [slice(0, 16), slice(16, 33)]):
        other, count = device_state(sc, *args, cuts=cuts)
        np.testing.assert_array_equal(BITS(other), BITS(once))
        np.testing.assert_array_equal(count, seen)


# ------------------------------------------------------------------------------------------------ 2. resolve, counts, the color_fn
def test_resolve_and_call_equal_restatement():
    args = ('nerfstudio', 'z', True, 2)
    sc = V.edge_scene(17, 'nerfstudio', 'z')
    state, seen = restated(17, *args)
    rng = np.random.default_rng(3)
    fb = rng.random((V.NPTS, 3)).astype(np.float32)
    fill = (0.125, 0.5, 0.75)
    x, d = cuda(sc['points']), cuda(-sc['normals'])
    # without a fallback: the fill colour
    vc = view_colors(sc, *args, fill=fill)
    want, counts = V.resolve(state, seen, None, fill)
    assert counts.sum() == V.NPTS and (counts > 0).all()
    np.testing.assert_array_equal(BITS(host(vc(x, d))), BITS(want))
    np.testing.assert_array_equal(host(vc.counts), counts)
    np.testing.assert_array_equal(BITS(host(vc.resolve(cuda(state), cuda(seen.astype(np.int32))))), BITS(want))
    np.testing.assert_array_equal(host(vc.counts), 2 * counts)                   # the tallies add up over the calls ...
    empty = vc(x[:0], d[:0])
    assert tuple(empty.shape) == (0, 3) and np.array_equal(host(vc.counts), 2 * counts)
    vc.reset_counts()
    assert not host(vc.counts).any()                                             # ... until they are cleared
    # with one: a color_fn with a fourth channel in float64, asked for the whole chunk
    asked = []

    def fallback(xq, dq):
        asked.append((xq.shape[0], bool(torch.equal(xq, x)), bool(torch.equal(dq, d))))
        return torch.cat([cuda(fb), torch.ones(V.NPTS, 1, device='cuda')], 1).double()
    vc = view_colors(sc, *args, fallback=fallback, fill=fill)
    want, counts = V.resolve(state, seen, fb, fill)
    np.testing.assert_array_equal(BITS(host(vc(x, d))), BITS(want))
    np.testing.assert_array_equal(host(vc.counts), counts)
    assert asked == [(V.NPTS, True, True)]
    with pytest.raises(ValueError):
        vc(x, d[:5])
    with pytest.raises(ValueError):
        vc.accumulate(x, -d, views=slice(0, 17, 2))


# ------------------------------------------------------------------------------------------------ 3. the sphere, end to end on the device
def test_sphere_end_to_end():
    """The polyhedron inscribed in the coloured sphere, its depth from mesh.rasterize, the ray-traced images of the 14 cameras: the device
    equals the restatement bit for bit, every vertex is seen, and the fused vertex colours lie within SPHERE_BOUND = 1.4e-3 of the analytic
    0.5 + 0.5 x / |x| (measured on the restatement, tests/test_mesh_view_colors_host.py: 6.6e-4; the bound is twice that)."""
    from customnerf_amd import mesh
    verts, faces, normals = V.sphere_mesh()
    cams, images = V.sphere_cameras(), V.sphere_images()
    v, f = cuda(verts), cuda(faces)
    depth = torch.stack([mesh.rasterize(v, f, c, V.INTRINSICS, V.IMG, V.IMG)['depth'] for c in cams])
    assert bool(torch.isinf(depth).any()) and bool((depth < 3).any())
    vc = mesh.ViewColors(cuda(images), depth, cams, V.INTRINSICS, V.SPHERE_TOL)
    state, seen = vc.accumulate(v, cuda(normals))
    want, count = V.fuse(verts, normals, images, host(depth), cams, V.INTRINSICS, V.SPHERE_TOL)
    np.testing.assert_array_equal(host(seen).astype(np.uint32), count)
    np.testing.assert_array_equal(BITS(host(state)), BITS(want))
    out = host(vc(v, -cuda(normals)))
    np.testing.assert_array_equal(BITS(out), BITS(V.resolve(want, count)[0]))
    err = np.abs(out.astype(np.float64) - V.sphere_color(verts.astype(np.float64))).max()
    print(f"{len(verts)} vertices seen by {count.min()} ... {count.max()} views, max colour error {err:.3e}, counts {host(vc.counts)}")
    assert count.min() >= 1 and host(vc.counts)[0] == 0
    assert err <= SPHERE_BOUND
    # through the baker: a texture of the sphere whose owned texels carry the analytic colour of their direction
    # (2 c - 1 is a unit vector: one view gives exactly that; blending views whose rays meet the chord's texel a little apart on the sphere
    # and interpolating between pixels 0.06 rad apart shorten it by under 3e-3, rounding to uint8 moves it by at most sqrt(3) / 255)
    vc.reset_counts()
    uvs, tex = mesh.bake_texture(v, f, 128, vc, normals=cuda(normals), fill=(255, 0, 255))
    texels = host(tex).reshape(-1, 3).astype(np.float64)
    owned = ~(texels == (255, 0, 255)).all(1)
    unit = np.linalg.norm(2.0 * texels[owned] / 255.0 - 1.0, axis=1)
    print(f"texture: {owned.sum()} owned texels, counts {host(vc.counts)}, |2 c - 1| in {unit.min():.4f} ... {unit.max():.4f}")
    assert owned.sum() > 128 * 128 // 4 and host(vc.counts)[0] == 0
    assert np.abs(unit - 1.0).max() <= 0.01


# ------------------------------------------------------------------------------------------------ 4. the renderer
RENDERERS = [(False, False), (True, False), (False, True), (True, True)]
IDS = ["fp32-run", "fp16-run", "fp32-march", "fp16-march"]
# the test field is hazy (tests/test_gpu_mesh_tsdf.py): 0.9 lies above the haze and below the blob
VIEWS = dict(poses=T.sphere_cameras(), intrinsics=T.INTRINSICS, H=T.IMG, W=T.IMG, min_opacity=0.9)
RES = 32
FACES = 400            # a 64 x 64 uniform atlas has 256 cells of 4 x 4 texels, room for 512 faces: the blob's 2252 are decimated to fit


def renderer(tcnn, fp16, cuda_ray):
    model = gaussian_model(tcnn, fp16, cuda_ray=cuda_ray)
    with torch.no_grad():
        model.aabb_infer.copy_(torch.tensor(AABB))                               # rays start at the box the mesh is taken from
    if cuda_ray:
        model.update_extra_state()
    return model


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(host(a.contiguous()).view(np.uint8), host(b.contiguous()).view(np.uint8))


@pytest.mark.parametrize("fp16, cuda_ray", RENDERERS, ids=IDS)
def test_render_view_matches_render_depth(dtype_guard, fp16, cuda_ray):
    model = renderer(dtype_guard, fp16, cuda_ray)
    pose, k = T.look_at((0.4, -1.1, 1.6)), (55.0, 50.0, 18.0, 14.0)
    for batch in (1 << 16, 500):                                                 # one ray batch, and three with a short last one
        a = model.render_view(pose, k, 30, 36, min_opacity=0.9, max_ray_batch=batch)
        b = model.render_depth(pose, k, 30, 36, min_opacity=0.9, max_ray_batch=batch)
        assert set(a) == {'image', 'depth', 'opacity'} and tuple(a['image'].shape) == (30, 36, 3) and a['image'].dtype == torch.float32
        assert same_bytes(a['depth'], b['depth']) and same_bytes(a['opacity'], b['opacity'])
        image = host(a['image'])
        assert np.isfinite(image).all() and image.min() >= 0.0 and image.max() <= 1.0 + 1e-3
        assert bool(torch.isinf(a['depth']).any()) and bool((a['depth'] < 3).any())


def by_hand(model, m, cfg, source, chunk=2 ** 21):
    """extract_mesh's colours composed from the public pieces: render_view and rasterize per pose, ViewColors with the field as fallback,
    then the vertex loop and bake_texture"""
    from customnerf_amd import mesh
    surface = source[:2] if source is not None else (m['verts'], m['faces'])
    images, depths, weights = [], [], []
    for pose in cfg['poses']:
        rv = model.render_view(pose, cfg['intrinsics'], cfg['H'], cfg['W'], min_opacity=cfg['min_opacity'])
        images.append(rv['image'])
        weights.append(torch.where(rv['opacity'] >= cfg['min_opacity'], rv['opacity'], torch.zeros_like(rv['opacity'])))
        depths.append(mesh.rasterize(*surface, pose, cfg['intrinsics'], cfg['H'], cfg['W'])['depth'])
    vc = mesh.ViewColors(torch.stack(images), torch.stack(depths), cfg['poses'], cfg['intrinsics'], cfg['depth_tol'], depth_kind='z',
                         weights=torch.stack(weights), power=cfg.get('power', 2), min_cos=cfg.get('min_cos', 0.2),
                         fallback=lambda x, d: model(x, d)[1][:, :3])
    x, look = m['verts'], -m['normals']
    src = None
    if source is not None:
        src = mesh.bake_source(*source)
        pr = mesh.project_to_surface(src, m['verts'], m['normals'], cfg['reach'])
        x, look = pr['point'], -pr['normal']
    colors = (vc(x.contiguous(), look.contiguous()).float().clamp(0, 1) * 255).round().to(torch.uint8)
    baked = mesh.bake_texture(m['verts'], m['faces'], 64, vc, normals=m['normals'], chunk=chunk, source=src,
                              reach=cfg['reach'] if src is not None else None)
    return colors, baked[1], vc


@pytest.mark.parametrize("bake_from", ["mesh", "source"])
def test_extract_mesh_color_views_equals_composition(dtype_guard, bake_from):
    with torch.no_grad():
        model = renderer(dtype_guard, False, False)
        step = float(model._mesh_lattice(RES, AABB)[1].max())
        # decimated: with bake_from='source' the final mesh is not the surface the queried points lie on
        kw = dict(resolution=RES, aabb=AABB, threshold=10.0, color=True, texture=64, bake_from=bake_from, target_faces=FACES)
        m = model.extract_mesh(color_views=VIEWS, **kw)
        assert set(m['view_colors']) == {'views', 'seen', 'depth_tol'} and m['view_colors']['views'] == 14
        assert m['view_colors']['depth_tol'] == 2.0 * step
        seen = host(m['view_colors']['seen'])
        # 14 cameras round a convex blob: every point faces one of them within about 35 degrees, so most points are seen
        assert seen.dtype == np.int64 and seen.shape == (3,) and seen[0] < seen.sum() / 2 and seen[2] > 0
        plain = model.extract_mesh(**kw)
        for k in ('verts', 'faces', 'normals', 'uvs'):
            assert same_bytes(m[k], plain[k]), k                                 # the geometry does not depend on where colour comes from
        assert not same_bytes(m['texture'], plain['texture']) and not same_bytes(m['colors'], plain['colors'])
        source = None
        if bake_from == 'source':
            v0, f0, n0 = mesh_after_marching_cubes(model)
            source = (v0, f0, n0)
        colors, tex, vc = by_hand(model, m, {**VIEWS, 'depth_tol': 2.0 * step, 'reach': 4.0 * step}, source)
        assert same_bytes(m['colors'], colors) and same_bytes(m['texture'], tex)
        np.testing.assert_array_equal(host(vc.counts), seen)
        # the fused colours are those of the renders: the field's colour is constant here, so they stay close to the field query's
        diff = (m['colors'].int() - plain['colors'].int()).abs().max().item()
        print(f"bake_from={bake_from}: seen {seen}, fused vs field vertex colours differ by at most {diff} / 255")


def mesh_after_marching_cubes(model):
    from customnerf_amd import mesh
    lo, step = model._mesh_lattice(RES, AABB)
    vol = model.density_volume(RES, AABB)
    return mesh.marching_cubes(vol, 10.0, spacing=step.tolist(), origin=lo.tolist())


def test_color_views_tsdf_and_writers(dtype_guard, tmp_path):
    with torch.no_grad():
        model = renderer(dtype_guard, False, False)
        kw = dict(resolution=RES, aabb=AABB, tsdf=VIEWS, color=True, texture=64, target_faces=FACES)
        a = model.extract_mesh(color_views='tsdf', **kw)
        b = model.extract_mesh(color_views=dict(VIEWS), **kw)
        for k in ('verts', 'faces', 'normals', 'colors', 'uvs', 'texture'):
            assert same_bytes(a[k], b[k]), k
        assert np.array_equal(host(a['view_colors']['seen']), host(b['view_colors']['seen'])) and 'tsdf' in a
        with pytest.raises(ValueError):
            model.extract_mesh(resolution=RES, aabb=AABB, color=True, color_views='tsdf')
        with pytest.raises(ValueError):
            model.extract_mesh(resolution=RES, aabb=AABB, color_views=VIEWS)
        tuned = model.extract_mesh(color_views={**VIEWS, 'power': 4, 'min_cos': 0.5, 'depth_tol': 0.01}, **kw)
        # stricter on every count: a third of a lattice step, while the depth under a footprint seen at 60 degrees changes by more
        ts, as_ = host(tuned['view_colors']['seen']), host(a['view_colors']['seen'])
        assert tuned['view_colors']['depth_tol'] == 0.01 and ts[0] >= as_[0] and ts[2] < as_[2] and ts.sum() == as_.sum()
        ply = model.save_mesh(str(tmp_path / "m.ply"), resolution=RES, aabb=AABB, threshold=10.0, color=True, color_views=VIEWS)
        back = R.read_ply(str(tmp_path / "m.ply"))
        assert 'view_colors' in ply and np.array_equal(back["colors"], host(ply['colors']))
        for ext in ("obj", "glb"):
            m = model.save_mesh(str(tmp_path / f"m.{ext}"), resolution=RES, aabb=AABB, threshold=10.0, texture=64, target_faces=FACES,
                                color_views=VIEWS)
            assert 'view_colors' in m and os.path.getsize(tmp_path / f"m.{ext}") > 1000
        assert os.path.exists(tmp_path / "m.png") and os.path.exists(tmp_path / "m.mtl")


def test_default_path_is_untouched(dtype_guard):
    with torch.no_grad():
        model = renderer(dtype_guard, False, False)
        kw = dict(resolution=RES, aabb=AABB, threshold=10.0, color=True, texture=64, target_faces=FACES)
        a = model.extract_mesh(**kw)
        b = model.extract_mesh(color_views=None, **kw)
        assert set(a) == set(b) and 'view_colors' not in a
        for k in ('verts', 'faces', 'normals', 'volume', 'colors', 'uvs', 'texture'):
            assert same_bytes(a[k], b[k]), k
