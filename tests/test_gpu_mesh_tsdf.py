"""GPU: TSDF fusion (csrc/mesh_tsdf.hip) against its NumPy restatement (tests/tsdf_restatement.py) — bit-equal state, volume and face flags —
the analytic sphere end to end through mesh.TSDFVolume, and extract_mesh(tsdf=...) / render_depth through NeRFNetwork."""
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
from mesh_testlib import AABB, cuda, dtype_guard, gaussian_model, host, octahedron_sphere  # noqa: E402,F401

BITS = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)             # noqa: E731

# the smallest shapes that can still go wrong: no extent a multiple of the 4 x 4 x 32 brick, an odd row length (pairs of points that are not
# 16-byte aligned, a last point without a partner), twenty workgroups, unequal spacing, images wider than high
SHAPE, ORG, SP, TRUNC = (19, 13, 11), (-0.5, -0.45, -0.4), (0.055, 0.075, 0.08), 0.22
H, W = 17, 24
K = (21.0, 19.0, 11.6, 8.3)
NPTS = SHAPE[0] * SHAPE[1] * SHAPE[2]


def to_ngp(c2w):
    """the same camera in the 'ngp' convention (+z forward, y down): columns y and z change sign"""
    m = np.array(c2w, np.float32)
    m[..., :3, 1:3] *= -1
    return m


@functools.lru_cache(maxsize=None)
def scene(n_views, convention):
    """(c2w [N, 3, 4], depth [N, H, W], weights [N, H, W]): cameras round the box looking at it, the second one inside it (points behind it
    and nearer than `near`); depths round the distance to the box, seeded with +inf, NaN, 0 and negative pixels; weights with zeros"""
    rng = np.random.default_rng(100 + n_views)
    eyes = rng.standard_normal((n_views, 3))
    eyes = eyes / np.linalg.norm(eyes, axis=1, keepdims=True) * rng.uniform(1.0, 1.6, (n_views, 1))
    eyes[1] = (0.05, -0.02, 0.03)
    cams = np.stack([T.look_at(e) for e in eyes])
    if convention == 'ngp':
        cams = to_ngp(cams)
    dist = np.linalg.norm(eyes, axis=1)[:, None, None]
    depth = (dist + rng.uniform(-0.45, 0.45, (n_views, H, W))).astype(np.float32)
    depth[1] = rng.uniform(0.05, 0.5, (H, W))
    kind = rng.random(depth.shape)
    depth[kind < 0.10] = np.inf
    depth[(kind >= 0.10) & (kind < 0.14)] = np.nan
    depth[(kind >= 0.14) & (kind < 0.17)] = 0.0
    depth[(kind >= 0.17) & (kind < 0.20)] = -0.7
    weights = rng.uniform(0.25, 2.0, depth.shape).astype(np.float32)
    weights[rng.random(depth.shape) < 0.15] = 0.0
    return cams, depth, weights


def device_state(cams, depth, weights, convention, kind, cuts=None, lattice=(SHAPE, ORG, SP, TRUNC)):
    from customnerf_amd import mesh
    tv = mesh.TSDFVolume(*lattice)
    for s in cuts or [slice(None)]:
        tv.integrate(cuda(depth[s]), cams[s], K, convention=convention, depth_kind=kind, weights=None if weights is None else cuda(weights[s]))
    assert tv.views == len(depth)
    return host(tv.state)


# ------------------------------------------------------------------------------------------------ 1. integrate, bit for bit
@pytest.mark.parametrize("n_views", [3, 17, 33])
@pytest.mark.parametrize("kind", ["ray", "z"])
@pytest.mark.parametrize("convention", ["nerfstudio", "ngp"])
def test_integrate_equals_restatement(convention, kind, n_views):
    cams, depth, weights = scene(n_views, convention)
    for w in (weights, None):
        want = T.integrate(np.zeros((NPTS, 2), np.float32), SHAPE, ORG, SP, TRUNC, depth, cams, K, convention, kind, w)
        got = device_state(cams, depth, w, convention, kind)
        seen = want[:, 1] > 0
        assert 0.3 * NPTS < seen.sum() <= NPTS and (want[seen, 0] > 0).any() and (want[seen, 0] < 0).any()   # inside and free points
        np.testing.assert_array_equal(BITS(got), BITS(want))


def test_integrate_several_bricks_along_z():
    """70 points along z: three workgroups a column, the last one partly filled; an even row length, so every pair is one wide access"""
    lattice = ((5, 6, 70), (-0.4, -0.4, -0.49), (0.2, 0.16, 0.0142), 0.2)
    cams, depth, weights = scene(17, 'nerfstudio')
    want = T.integrate(np.zeros((5 * 6 * 70, 2), np.float32), *lattice, depth, cams, K, 'nerfstudio', 'ray', weights)
    assert (want[:, 1] > 0).sum() > 1000 and (want[:, 0] > 0).any() and (want[:, 0] < 0).any()
    np.testing.assert_array_equal(BITS(device_state(cams, depth, weights, 'nerfstudio', 'ray', lattice=lattice)), BITS(want))


# ------------------------------------------------------------------------------------------------ 2. the cut into launches and calls
def test_batching_does_not_matter():
    cams, depth, weights = scene(33, 'nerfstudio')
    once = device_state(cams, depth, weights, 'nerfstudio', 'ray')
    again = device_state(cams, depth, weights, 'nerfstudio', 'ray')
    single = device_state(cams, depth, weights, 'nerfstudio', 'ray', cuts=[slice(v, v + 1) for v in range(33)])
    halves = device_state(cams, depth, weights, 'nerfstudio', 'ray', cuts=[slice(0, 16), slice(16, 33)])
    for other in (again, single, halves):
        np.testing.assert_array_equal(BITS(other), BITS(once))


def test_single_view_shapes():
    """depth [H, W] with c2w [4, 4] is one view; zero views leave the state alone"""
    from customnerf_amd import mesh
    cams, depth, _ = scene(3, 'nerfstudio')
    tv = mesh.TSDFVolume(SHAPE, ORG, SP, TRUNC)
    tv.integrate(cuda(depth[0]), np.concatenate([cams[0], [[0, 0, 0, 1]]]).astype(np.float32), K)
    tv.integrate(cuda(depth[:0]), cams[:0], K)
    want = T.integrate(np.zeros((NPTS, 2), np.float32), SHAPE, ORG, SP, TRUNC, depth[:1], cams[:1], K)
    assert tv.views == 1
    np.testing.assert_array_equal(BITS(host(tv.state)), BITS(want))
    with pytest.raises(ValueError):
        tv.integrate(cuda(depth), cams[:2], K)
    with pytest.raises(ValueError):
        tv.integrate(cuda(depth[0]), cams[0], K, depth_kind='disparity')


# ------------------------------------------------------------------------------------------------ 3. finalize and the face rule
def test_finalize_and_face_rule_equal_restatement():
    from customnerf_amd import mesh
    rng = np.random.default_rng(5)
    state = np.stack([rng.standard_normal(NPTS), rng.uniform(0.5, 3.0, NPTS)], 1).astype(np.float32)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in SHAPE], indexing="ij"), -1).reshape(-1, 3)
    smooth = np.sin(idx[:, 0] * 0.7) + np.cos(idx[:, 1] * 0.9) + np.sin(idx[:, 2] * 0.8 + 1.0)
    state[:, 0] = (smooth * state[:, 1]).astype(np.float32) + state[:, 0] * np.float32(0.1)
    state[rng.random(NPTS) < 0.3] = 0.0                                          # about 30 % unobserved
    tv = mesh.TSDFVolume(SHAPE, ORG, SP, TRUNC)
    tv.state.copy_(cuda(state))
    for fill in (-1.0, 0.25):
        want, count = T.finalize(state, SHAPE, fill)
        np.testing.assert_array_equal(BITS(host(tv.volume(fill))), BITS(want))
        assert abs(tv.observed - count / NPTS) < 1e-12 and 0.6 < tv.observed < 0.8
    vol = tv.volume()
    v, f, _ = mesh.marching_cubes(vol, 0.0, spacing=SP, origin=ORG, normals=False)
    keep = T.face_keep(state, SHAPE, ORG, SP, host(v), host(f))
    assert 50 < keep.sum() < 0.2 * len(keep)                                      # 0.7^8 of the cells have eight observed corners
    np.testing.assert_array_equal(host(tv.face_keep(v, f)), keep)
    wv, wf = T.compact(host(v), host(f), keep)
    gv, gf, gn, info = tv.extract()
    np.testing.assert_array_equal(BITS(host(gv)), BITS(wv))
    np.testing.assert_array_equal(host(gf), wf)                                  # the surviving faces in their order
    np.testing.assert_array_equal(BITS(host(gn)), BITS(host(mesh.vertex_normals(cuda(wv), cuda(wf)))))
    assert info == {'observed': count / NPTS, 'dropped_faces': int(len(keep) - keep.sum())}


# ------------------------------------------------------------------------------------------------ 4. the sphere, end to end on the device
def closed_single_component(v, f):
    from customnerf_amd import mesh
    assert R.check_closed_oriented(host(v), host(f)) == 0                        # every edge used twice, once in each direction
    v2, f2, _, _ = mesh.remove_small_components(v, f, largest=True)
    assert v2.shape == v.shape and f2.shape == f.shape                           # one connected component


def fused_sphere(kind, depth):
    from customnerf_amd import mesh
    tv = mesh.TSDFVolume(T.SHAPE, T.ORIGIN, T.SPACING, T.TRUNC)
    tv.integrate(depth, T.sphere_cameras(), T.INTRINSICS, depth_kind=kind)
    return tv, tv.extract()


def test_sphere_end_to_end():
    from customnerf_amd import mesh
    cams = T.sphere_cameras()
    for kind in ("ray", "z"):
        tv, (v, f, n, info) = fused_sphere(kind, cuda(np.stack([T.sphere_depth(c, kind) for c in cams])))
        np.testing.assert_array_equal(BITS(host(tv.state)), BITS(T.fuse_sphere(kind)))
        hv, hf = host(v).astype(np.float64), host(f)
        err = np.abs(np.linalg.norm(hv, axis=1) - T.RADIUS) / T.STEP
        print(f"{kind}: {len(hv)} vertices, {len(hf)} faces, max |r - R| {err.max():.3f} steps, dropped {info['dropped_faces']}")
        assert len(hf) > 1000 and err.max() <= 0.5                               # the restatement's bound (tests/test_mesh_tsdf_host.py)
        closed_single_component(v, f)
        assert info['dropped_faces'] > 0 and 0.9 < info['observed'] < 1.0        # the inner shell existed and is gone
        assert ((R.face_normals(hv, hf) * hv[hf].mean(1)).sum(1) > 0).all()      # wound outwards
        assert ((host(n) * hv).sum(1) > 0).all()
        if kind == "z":
            analytic = (v, f)
    # the same through the rasteriser: camera-axis depth of a polyhedron inscribed in the sphere
    ov, of = octahedron_sphere(3)
    ov, of = cuda((ov * T.RADIUS).astype(np.float32)), cuda(of)
    depth = torch.stack([mesh.rasterize(ov, of, c, T.INTRINSICS, T.IMG, T.IMG)['depth'] for c in cams])
    assert bool(torch.isinf(depth).any()) and bool((depth < 3).any())
    _, (v, f, n, info) = fused_sphere("z", depth)
    closed_single_component(v, f)
    d = mesh.distance(v, f, analytic[0], analytic[1])
    print(f"rasterised against analytic depth: hausdorff {d['hausdorff'] / T.STEP:.3f} steps")
    assert d['hausdorff'] <= T.STEP


# ------------------------------------------------------------------------------------------------ 5. the renderer
RENDERERS = [(False, False), (True, False), (False, True), (True, True)]
# The test field's density is exp(5 exp(-|x|^2 / 0.08)) >= 1 everywhere: a haze whose opacity across the box reaches about 0.85, which the
# default min_opacity = 0.5 would take for a surface.  0.9 lies above the haze and below the blob.
TSDF = dict(poses=T.sphere_cameras(), intrinsics=T.INTRINSICS, H=T.IMG, W=T.IMG, min_opacity=0.9)


def renderer(tcnn, fp16, cuda_ray):
    model = gaussian_model(tcnn, fp16, cuda_ray=cuda_ray)
    with torch.no_grad():
        model.aabb_infer.copy_(torch.tensor(AABB))                               # rays start at the box the mesh is taken from
    if cuda_ray:
        model.update_extra_state()
    return model


@pytest.mark.parametrize("fp16, cuda_ray", RENDERERS, ids=["fp32-run", "fp16-run", "fp32-march", "fp16-march"])
def test_render_depth_is_metric(dtype_guard, fp16, cuda_ray):
    model = renderer(dtype_guard, fp16, cuda_ray)
    r = model.render_depth(T.look_at((0, 0, 2)), (55.0, 55.0, 16.0, 16.0), 32, 32)
    depth, opacity = host(r['depth']), host(r['opacity'])
    assert depth.shape == opacity.shape == (32, 32) and depth.dtype == np.float32
    centre = depth[15:17, 15:17]
    print(f"centre depth {centre.ravel()}, opacity {opacity[15:17, 15:17].ravel()}, corner opacity {opacity[0, 0]:.3f}")
    assert (centre > 1.5).all() and (centre < 2.0).all()                         # box entry ... the blob's centre; a normalised depth is <= 1
    assert (opacity[15:17, 15:17] > 0.99).all()
    for corner in (depth[0, 0], depth[0, -1], depth[-1, 0], depth[-1, -1]):
        assert corner == np.inf                                                  # haze only: below min_opacity
    assert (opacity >= 0).all() and (opacity <= 1.0 + 1e-4).all()


@pytest.mark.parametrize("fp16, cuda_ray", RENDERERS, ids=["fp32-run", "fp16-run", "fp32-march", "fp16-march"])
def test_extract_mesh_tsdf(dtype_guard, fp16, cuda_ray):
    model = renderer(dtype_guard, fp16, cuda_ray)
    maps, render_depth = [], model.render_depth

    def recording(*a, **k):
        out = render_depth(*a, **k)
        maps.append(host(out['depth']).copy())
        return out
    model.render_depth = recording
    m = model.extract_mesh(resolution=T.RES, aabb=AABB, tsdf=TSDF)
    del model.render_depth
    assert len(maps) == 14 and m['threshold'] == 0.0 and tuple(m['volume'].shape) == T.SHAPE
    assert set(m['tsdf']) == {'views', 'trunc', 'observed', 'dropped_faces'} and m['tsdf']['views'] == 14
    assert m['tsdf']['trunc'] == 4.0 * float(np.float32(1.0) / np.float32(T.RES - 1)) and m['tsdf']['dropped_faces'] > 0
    lo, step = model._mesh_lattice(T.RES, AABB)
    state = T.integrate(np.zeros((T.RES ** 3, 2), np.float32), T.SHAPE, lo.tolist(), step.tolist(), m['tsdf']['trunc'], np.stack(maps),
                        TSDF['poses'], T.INTRINSICS, 'nerfstudio', 'ray')
    want, count = T.finalize(state, T.SHAPE)
    np.testing.assert_array_equal(BITS(host(m['volume'])), BITS(want))
    assert m['tsdf']['observed'] == count / T.RES ** 3
    closed_single_component(m['verts'], m['faces'])
    r = np.linalg.norm(host(m['verts']).astype(np.float64), axis=1)
    print(f"fused blob: radius {r.min():.3f} ... {r.max():.3f}, {len(r)} vertices")
    assert 0.2 < r.min() and r.max() < 0.4                                       # a ball round the blob, not the box or the haze
    assert ((host(m['normals']) * host(m['verts'])).sum(1) > 0).all()


def test_extract_mesh_tsdf_options_and_later_stages(dtype_guard, tmp_path):
    model = renderer(dtype_guard, False, False)
    for bad in (dict(sparse=True), dict(part='fg')):
        with pytest.raises(ValueError):
            model.extract_mesh(resolution=T.RES, aabb=AABB, tsdf=TSDF, **bad)
    for bad in (dict(trunc=0.0), dict(poses=TSDF['poses'][:0]), dict(colour=1)):
        with pytest.raises(ValueError):
            model.extract_mesh(resolution=T.RES, aabb=AABB, tsdf={**TSDF, **bad})
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=T.RES, aabb=AABB, tsdf={k: v for k, v in TSDF.items() if k != 'H'})
    p = str(tmp_path / "m.ply")
    m = model.save_mesh(p, resolution=T.RES, aabb=AABB, tsdf=TSDF, target_faces=600, color=True)
    back = R.read_ply(p)
    assert 'tsdf' in m and 0 < len(back["faces"]) <= 600
    assert np.array_equal(back["verts"], host(m['verts'])) and np.array_equal(back["faces"], host(m['faces']))
    assert back["colors"].dtype == np.uint8 and back["colors"].shape == (len(back["verts"]), 3) and np.isfinite(back["normals"]).all()
    # carve=False: transparent pixels say nothing, so fewer points are observed
    kept = model.extract_mesh(resolution=T.RES, aabb=AABB, tsdf={**TSDF, 'carve': False})
    assert kept['tsdf']['observed'] < m['tsdf']['observed']


def test_default_path_is_untouched(dtype_guard):
    model = renderer(dtype_guard, False, False)
    a = model.extract_mesh(resolution=48, threshold=10.0, aabb=AABB)
    b = model.extract_mesh(resolution=48, threshold=10.0, aabb=AABB, tsdf=None)
    assert set(a) == set(b) and 'tsdf' not in a and a['threshold'] == b['threshold'] == 10.0
    for k in ('verts', 'faces', 'normals', 'volume'):
        assert a[k].dtype == b[k].dtype and np.array_equal(host(a[k]).view(np.uint8), host(b[k]).view(np.uint8)), k
