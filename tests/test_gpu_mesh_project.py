"""GPU: the projection query through the mesh BVH (csrc/mesh_bvh.hip, k_bvh_project) against its NumPy restatement
(tests/project_restatement.py) bit for bit — kind, face, offset, point and normal on the atlas texels of a coarse icosphere, with and without source
normals; against the project's own ray_cast and closest_point kernels on marching-cubes meshes; the pruning of the narrowed second walk;
the thin slab, the rim, opposed source normals — and the layers above it: bake_texture(source=, normal_map=), extract_mesh(bake_from=,
normal_map=), save_mesh and render_mesh(map=)."""
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
import project_restatement as P  # noqa: E402
import project_testlib as L  # noqa: E402
import ray_testlib as T  # noqa: E402
from mesh_testlib import AABB, cuda, dtype_guard, gaussian_model, grid  # noqa: E402,F401

F32 = np.float32
SENTINEL = -7.0
PAD = 8
FLOATS = ('offset', 'point', 'normal')


def gpu_tree(v, f, normals=None):
    """cnerf_mesh_bvh_build -> (ws, nbytes, V, F, faces, normals on the device)"""
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib, check, ptr, stream
    gv, gf = cuda(np.asarray(v, F32)), cuda(np.asarray(f, np.int32))
    V, F = len(v), len(f)
    nbytes = mesh.bvh_workspace_bytes(V, F)
    ws = torch.full((nbytes + 256,), 0x5a, dtype=torch.uint8, device="cuda")
    counts = torch.empty(2, dtype=torch.int32, device="cuda")
    check(lib.cnerf_mesh_bvh_build(ptr(gv) if V else None, V, ptr(gf) if F else None, F, ptr(ws), nbytes, ptr(counts), stream()), "build")
    return ws, nbytes, V, F, gf, cuda(None if normals is None else np.asarray(normals, F32))


def gpu_project(tree, x, n, reach, want=("point", "normal", "offset", "face", "kind", "stats")):
    """cnerf_mesh_bvh_project into sentinel-padded buffers -> dict of arrays without the (checked) padding; the workspace is checked too"""
    from customnerf_amd._lib import lib, check, ptr, stream
    ws, nbytes, V, F, gf, gn = tree
    before = ws.clone()
    Q = len(x)
    gx, gd = cuda(np.asarray(x, F32).reshape(-1, 3)), cuda(np.asarray(n, F32).reshape(-1, 3))
    r0, per = (float(reach), None) if np.ndim(reach) == 0 else \
        (0.0, torch.cat([cuda(np.asarray(reach, F32)), torch.full((PAD,), SENTINEL, device="cuda")]))
    buf = {'point': torch.full((3 * Q + PAD,), SENTINEL, device="cuda"), 'normal': torch.full((3 * Q + PAD,), SENTINEL, device="cuda"),
           'offset': torch.full((Q + PAD,), SENTINEL, device="cuda"), 'face': torch.full((Q + PAD,), int(SENTINEL), dtype=torch.int32, device="cuda"),
           'kind': torch.full((Q + PAD,), 0x5a, dtype=torch.uint8, device="cuda"), 'stats': torch.zeros(2 + PAD, dtype=torch.int64, device="cuda")}
    p = lambda k: ptr(buf[k]) if k in want else None                              # noqa: E731
    check(lib.cnerf_mesh_bvh_project(ptr(ws), nbytes, V, F, ptr(gf) if F else None, None if gn is None else ptr(gn), ptr(gx) if Q else None,
                                     ptr(gd) if Q else None, Q, r0, None if per is None else ptr(per), p('point'), p('normal'), p('offset'),
                                     p('face'), p('kind'), p('stats'), stream()), "project")
    torch.cuda.synchronize()
    assert torch.equal(ws, before)                                                # a query writes nothing into the tree or past it
    out = {}
    for k, m, s in (('point', 3, SENTINEL), ('normal', 3, SENTINEL), ('offset', 1, SENTINEL), ('face', 1, int(SENTINEL)), ('kind', 1, 0x5a)):
        a = buf[k].cpu().numpy()
        if k in want:
            assert (a[m * Q:] == s).all(), k
            out[k] = a[:m * Q].reshape((Q, 3) if m == 3 else (Q,))
        else:
            assert (a == s).all(), k                                              # an output that was not asked for is not written
    s = buf['stats'].cpu().numpy()
    assert (s[2:] == 0).all()
    if 'stats' in want:
        out['stats'] = (int(s[0]), int(s[1]))
    return out


def assert_same(got, want, rows=slice(None)):
    for k in ('kind', 'face'):
        if k in got:
            np.testing.assert_array_equal(got[k], want[k][rows], err_msg=k)
    for k in FLOATS:
        if k in got:
            np.testing.assert_array_equal(got[k].view(np.uint32), want[k][rows].view(np.uint32), err_msg=k)


@pytest.mark.parametrize("reach", [0.25, 0.02])
def test_sphere_matches_restatement(reach):
    """the 3240 atlas texels of the 80-face icosphere against the 1280-face one: kind, face, offset, point and normal bit-equal to the
    restatement (whose counts and radii tests/test_mesh_project_host.py pins); outputs left NULL are not written; query counts 0 and 1"""
    s = L.sphere()
    want = L.sphere_want(reach)
    tree = gpu_tree(s['sv'], s['sf'], s['sv'])
    got = gpu_project(tree, s['x'], s['n'], reach)
    print(f"reach {reach}: kinds {P.kinds(got['kind']).tolist()}, {got['stats'][1] / len(s['x']):.1f} triangle and "
          f"{got['stats'][0] / len(s['x']):.1f} box tests per query")
    assert P.kinds(got['kind']).tolist() == ([0, 2920, 320, 0] if reach == 0.25 else [2340, 740, 160, 0])
    assert_same(got, want)
    rad = np.linalg.norm(got['point'][got['kind'] > 0].astype(np.float64), axis=1)
    assert rad.min() >= s['inradius'] - 1e-6 and rad.max() <= 1.0 + 1e-6
    none = got['kind'] == 0
    np.testing.assert_array_equal(got['point'][none].view(np.uint32), s['x'][none].view(np.uint32))
    # a per-query reach gives the same; a subset of the outputs gives the same and writes nothing else
    assert_same(gpu_project(tree, s['x'], s['n'], np.full(len(s['x']), reach, F32)), want)
    assert_same(gpu_project(tree, s['x'], s['n'], reach, want=("kind", "offset")), want)
    assert_same(gpu_project(tree, s['x'], s['n'], reach, want=("normal",)), want)
    for Q in (0, 1):
        assert_same(gpu_project(tree, s['x'][:Q], s['n'][:Q], reach), want, slice(0, Q))
    assert gpu_project(tree, s['x'][:0], s['n'][:0], reach)['stats'] == (0, 0)


def test_sphere_without_source_normals():
    """source normals NULL: the hit faces' own normals, bit for bit; everything else as with them"""
    s = L.sphere()
    want = L.sphere_want(0.25, False)
    got = gpu_project(gpu_tree(s['sv'], s['sf'], None), s['x'], s['n'], 0.25)
    assert_same(got, want)
    with_n = L.sphere_want(0.25)
    for k in ('kind', 'face', 'offset', 'point'):
        np.testing.assert_array_equal(want[k], with_n[k])
    assert (want['normal'] != with_n['normal']).any()


def test_second_walk_is_narrowed():
    """on the sphere case with reach 0.25 every query hits with a ray, so no closest-point walk runs, and one project call tests no more
    boxes and no more triangles than the two ray_cast calls it stands for: the second walk's range ends at the first hit"""
    from customnerf_amd import mesh
    s = L.sphere()
    src = mesh.bake_source(cuda(s['sv']), cuda(s['sf']), cuda(s['sv']))
    x, n = cuda(s['x']), cuda(s['n'])
    pr = mesh.project_to_surface(src, x, n, 0.25, want_stats=True)
    assert int((pr['kind'] == 0).sum()) == 0 and int((pr['kind'] == 3).sum()) == 0
    fw = mesh.ray_cast(src.bvh, x, n, 0.0, 0.25, cull='front', want_stats=True)
    bw = mesh.ray_cast(src.bvh, x, -n, 0.0, 0.25, cull='back', want_stats=True)
    print(f"boxes {pr['stats'][0]} against {fw['stats'][0]} + {bw['stats'][0]}, triangles {pr['stats'][1]} against {fw['stats'][1]} + "
          f"{bw['stats'][1]}")
    assert pr['stats'][0] <= fw['stats'][0] + bw['stats'][0] and pr['stats'][1] <= fw['stats'][1] + bw['stats'][1]
    assert pr['stats'][0] > 0 and pr['stats'][1] > 0


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_against_ray_cast_and_closest_point(name):
    """marching-cubes meshes, their vertices moved along +- their normals by up to twice the reach, behind the degenerate rays of the ray
    tests: kinds 1 and 2 are the better of ray_cast(cull 'front') along n and ray_cast(cull 'back') along -n, bit for bit; kind 3 is
    closest_point where both miss and it lies within reach; kind 0 everything else"""
    from customnerf_amd import mesh
    v, f = T.mesh(name)
    gv, gf = cuda(v), cuda(f)
    nv = mesh.vertex_normals(gv, gf)
    reach = 0.04
    x, n = L.displaced(name, reach)(nv.cpu().numpy())
    src = mesh.bake_source(gv, gf, nv)
    gx, gn = cuda(x), cuda(n)
    pr = {k: t.cpu().numpy() for k, t in mesh.project_to_surface(src, gx, gn, reach).items()}
    fw = {k: t.cpu().numpy() for k, t in mesh.ray_cast(src.bvh, gx, gn, 0.0, reach, cull='front').items()}
    bw = {k: t.cpu().numpy() for k, t in mesh.ray_cast(src.bvh, gx, -gn, 0.0, reach, cull='back').items()}
    cl = {k: t.cpu().numpy() for k, t in mesh.closest_point(src.bvh, gx, want_point=True).items()}
    hf, hb = fw['face'] >= 0, bw['face'] >= 0
    with np.errstate(all="ignore"):
        live = np.isfinite(x).all(1) & np.isfinite(n).all(1) & (n != 0).any(1)
        back = hb & (~hf | (bw['t'] < fw['t']))
        front = hf & ~back
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        near = live & ~hf & ~hb & (cl['face'] >= 0) & (cl['dist2'] <= (F32(reach) * F32(reach)) * nn)
    kind = np.where(front, 1, np.where(back, 2, np.where(near, 3, 0)))
    print(f"{name}: {len(x)} queries over {len(f)} faces, kinds {P.kinds(kind).tolist()}")
    assert min(P.kinds(kind)) > 20                                                # every kind occurs
    np.testing.assert_array_equal(pr['kind'], kind)
    assert (pr['kind'][:T.N_DEGENERATE - 2] == 0).all()                           # non-finite or zero: nothing (the last two are proper queries)
    for sel, r, sign in ((front, fw, F32(1)), (back, bw, F32(-1))):
        np.testing.assert_array_equal(pr['face'][sel], r['face'][sel])
        np.testing.assert_array_equal(pr['offset'][sel].view(np.uint32), (sign * r['t'][sel]).view(np.uint32))
    np.testing.assert_array_equal(pr['face'][near], cl['face'][near])
    np.testing.assert_array_equal(pr['point'][near].view(np.uint32), cl['point'][near].view(np.uint32))
    none = kind == 0
    assert (pr['face'][none] == -1).all() and (pr['offset'][none] == 0).all()
    np.testing.assert_array_equal(pr['point'][none].view(np.uint32), x[none].view(np.uint32))
    # and a seeded sample of it against the restatement, every output
    rows = np.concatenate([np.arange(T.N_DEGENERATE), np.random.default_rng(2).permutation(len(x))[:160]])
    want = P.project(v, f, nv.cpu().numpy(), x[rows], n[rows], reach)
    assert_same({k: pr[k][rows] for k in ('kind', 'face') + FLOATS}, want)


def test_thin_slab():
    """a wall 0.05 thick: above it, inside it and 0.01 over its bottom sheet, looking up, every query lands on the top sheet — an
    implementation that ignores the cull lands on the bottom sheet from 0.01"""
    v, f = L.slab()
    tree = gpu_tree(v, f)
    for z, off, kind in L.SLAB_HEIGHTS:
        x, n = L.slab_queries(z)
        got = gpu_project(tree, x, n, L.SLAB_REACH)
        assert (got['kind'] == kind).all() and (got['face'] >= 0).all() and (got['face'] < 32).all(), z
        assert np.abs(got['offset'] - off).max() < 1e-6 and np.abs(got['point'][:, 2] - 0.05).max() < 1e-6
        assert_same(got, P.project(v, f, None, x, n, L.SLAB_REACH))


def test_rim():
    """beside the sheet both rays miss: the closest point within reach (kind 3, face 3, (0, 2, 0): dist2 = 0.0125 <= 0.04), nothing with
    reach 0.1; |n| scales the reach"""
    v, f = grid(4)
    tree = gpu_tree(v, f)
    got = gpu_project(tree, L.RIM_X, L.RIM_N, 0.2)
    assert got['kind'][0] == 3 and got['face'][0] == 3 and got['point'][0].tolist() == [0.0, 2.0, 0.0]
    assert_same(got, P.project(v, f, None, L.RIM_X, L.RIM_N, 0.2))
    got = gpu_project(tree, L.RIM_X, L.RIM_N, 0.1)
    assert got['kind'][0] == 0 and got['face'][0] == -1
    np.testing.assert_array_equal(got['point'].view(np.uint32), L.RIM_X.view(np.uint32))
    for reach in (0.05, 0.025):
        assert_same(gpu_project(tree, L.RIM_X, 4 * L.RIM_N, reach), P.project(v, f, None, L.RIM_X, 4 * L.RIM_N, reach))


def test_opposed_source_normals():
    """vertex normals that cancel on the hit face, or are not finite: the face's normal; where nothing is found the query's own"""
    v, f, nrm, x, n = L.opposed()
    tree = gpu_tree(v, f, nrm)
    got = gpu_project(tree, x, n, 1.0)
    assert got['kind'].tolist() == [2, 2, 2]
    np.testing.assert_array_equal(got['normal'][1:], np.array([[1, 0, 0], [1, 0, 0]], F32))
    assert_same(got, P.project(v, f, nrm, x, n, 1.0))
    far = x + np.array([9, 0, 0], F32)
    assert_same(gpu_project(tree, far, n, 1.0), P.project(v, f, nrm, far, n, 1.0))
    # an empty tree finds nothing
    got = gpu_project(gpu_tree(v, f[:0]), x, n, 1.0)
    assert (got['kind'] == 0).all() and got['stats'] == (0, 0)
    np.testing.assert_array_equal(got['point'].view(np.uint32), x.view(np.uint32))


def shell_colour(x, d):
    """clamp((|x| - 0.9) / 0.2) in every channel: what a field trained on the unit sphere's shell might hold"""
    return ((x.norm(dim=1, keepdim=True) - 0.9) / 0.2).clamp(0, 1).expand(-1, 3)


@pytest.mark.parametrize("layout", ["uniform", "area", "projected"])
def test_bake_from_source(layout):
    """bake_texture of the 80-face icosphere with the 1280-face one as its source: every owned texel's colour is that of a point of the
    source's surface, radius in [r_in, 1], within 1 of the store's rounding; the bake without a source is not (its texels lie down to
    radius 0.934).  The normal map is the restatement's normals through the store's rounding, bit for bit; the kinds are its counts.
    Where the chunks fall changes no byte.  The projected layout is baked without a gutter: grown texels extrapolate beyond the reach"""
    from customnerf_amd import mesh
    s = L.sphere()
    lv, lf = cuda(s['lv']), cuda(s['lf'])
    src = mesh.bake_source(cuda(s['sv']), cuda(s['sf']), cuda(s['sv']))
    R = L.R_SPHERE
    kw = dict(normals=lv, layout=layout, **({'gutter': 0} if layout == 'projected' else {}))
    uvs, tex, extra = mesh.bake_texture(lv, lf, R, shell_colour, source=src, reach=0.25, normal_map=True, chunk=1000, **kw)
    _, tex1, extra1 = mesh.bake_texture(lv, lf, R, shell_colour, source=src, reach=0.25, normal_map=True, **kw)
    assert torch.equal(tex1, tex) and torch.equal(extra1['normal_map'], extra['normal_map']) and torch.equal(extra1['kinds'], extra['kinds'])
    plain = mesh.bake_texture(lv, lf, R, shell_colour, **kw)
    assert len(plain) == 2 and torch.equal(plain[0], uvs)
    lo, hi = round(255 * (s['inradius'] - 0.9) / 0.2), 128
    tex, nmap, old = tex.cpu().numpy(), extra['normal_map'].cpu().numpy(), plain[1].cpu().numpy()
    if layout == 'uniform':
        owned = A.owner_map(len(s['lf']), R) >= 0
        want = L.sphere_want(0.25)
        want_map = np.full((R, R, 3), 128, np.uint8)
        want_map[s['Y'], s['X']] = P.normal_texels(want['normal'])
        np.testing.assert_array_equal(nmap, want_map)
        assert extra['kinds'].cpu().tolist() == P.kinds(want['kind']).tolist()
    else:
        owned = (nmap != 128).any(2)                                              # a unit normal never maps to (128, 128, 128)
        assert owned.sum() > 1000 and int(extra['kinds'].sum()) >= owned.sum() and int(extra['kinds'][0]) == 0
    px = tex[owned].astype(np.int64)
    print(f"{layout}: baked from the source {px.min()} .. {px.max()} (allowed {lo - 1} .. {hi + 1}); from the mesh itself "
          f"{old[owned].min()} .. {old[owned].max()}")
    assert px.min() >= lo - 1 and px.max() <= hi + 1
    assert old[owned].min() < lo - 1                                              # what the feature changes
    assert (tex[~owned] == 0).all() and (nmap[~owned] == 128).all()
    # without a source the normal map holds the mesh's own interpolated normals
    _, tex2, extra2 = mesh.bake_texture(lv, lf, R, shell_colour, normal_map=True, **kw)
    assert np.array_equal(tex2.cpu().numpy(), old) and extra2['kinds'].cpu().tolist() == [0, 0, 0, 0]
    if layout == 'uniform':
        own_map = np.full((R, R, 3), 128, np.uint8)
        own_map[s['Y'], s['X']] = P.normal_texels(s['n'])
        np.testing.assert_array_equal(extra2['normal_map'].cpu().numpy(), own_map)


def test_extract_mesh_bakes_from_source(dtype_guard, tmp_path):
    """extract_mesh(target_faces=200, texture=64, bake_from='source', normal_map=True, color=True): the new keys with their shapes,
    bake_kinds equal to the restatement run on the downloaded meshes, no new key with the defaults; save_mesh writes <stem>_normal.png
    and refuses a PLY path; render_mesh(map='normal_map') shows the map"""
    from customnerf_amd import scene
    model = gaussian_model(dtype_guard, False)
    res = 28
    kw = dict(resolution=res, threshold=10.0, aabb=AABB)
    base = model.extract_mesh(**kw)
    assert 'normal_map' not in base and 'bake_kinds' not in base
    low = dict(target_faces=200, texture=64, color=True, **kw)
    plain = model.extract_mesh(**low)
    assert 'normal_map' not in plain and 'bake_kinds' not in plain
    m = model.extract_mesh(bake_from='source', normal_map=True, **low)
    F = m['faces'].shape[0]
    assert 0 < F < base['faces'].shape[0] // 2 and torch.equal(m['verts'], plain['verts']) and torch.equal(m['faces'], plain['faces'])
    assert tuple(m['normal_map'].shape) == (64, 64, 3) and m['normal_map'].dtype == torch.uint8
    assert tuple(m['bake_kinds'].shape) == (4,) and m['bake_kinds'].dtype == torch.int64
    assert tuple(m['colors'].shape) == (m['verts'].shape[0], 3) and tuple(m['texture'].shape) == (64, 64, 3)
    step = F32(1.0) / F32(res - 1)                                                # the lattice step of AABB, as _mesh_lattice makes it
    x, d = A.points(m['verts'].cpu().numpy(), m['faces'].cpu().numpy(), 64, normals=m['normals'].cpu().numpy())
    want = P.project(base['verts'].cpu().numpy(), base['faces'].cpu().numpy(), base['normals'].cpu().numpy(), x, -d, F32(4.0) * step)
    print(f"{len(x)} texels of {F} faces against {base['faces'].shape[0]}: kinds {P.kinds(want['kind']).tolist()}")
    assert m['bake_kinds'].cpu().tolist() == P.kinds(want['kind']).tolist()
    assert int(m['bake_kinds'][0]) < len(x) // 20                                 # the default reach covers what decimation moved
    face, _, _, X, Y = A.cell_texels(F, 64)
    want_map = np.full((64, 64, 3), 128, np.uint8)
    want_map[Y[face >= 0], X[face >= 0]] = P.normal_texels(want['normal'])[face >= 0]
    np.testing.assert_array_equal(m['normal_map'].cpu().numpy(), want_map)
    # without a lossy pass the projections are near zero: (almost) nothing is out of reach
    same = model.extract_mesh(bake_from='source', color=True, **kw)
    assert 'normal_map' not in same and int(same['bake_kinds'].sum()) == same['verts'].shape[0] and int(same['bake_kinds'][0]) == 0
    with pytest.raises(ValueError):
        model.extract_mesh(bake_from='surface', **kw)
    with pytest.raises(ValueError):
        model.extract_mesh(normal_map=True, **kw)                                 # no atlas to share
    path = str(tmp_path / "low.obj")
    s = model.save_mesh(path, bake_from='source', normal_map=True, **low)
    np.testing.assert_array_equal(A.read_png(str(tmp_path / "low_normal.png")), s['normal_map'].cpu().numpy())
    assert "norm low_normal.png\n" in open(str(tmp_path / "low.mtl")).read()
    with pytest.raises(ValueError):
        model.save_mesh(str(tmp_path / "low.ply"), normal_map=True, **kw)
    assert not os.path.exists(str(tmp_path / "low.ply"))
    c2w = np.asarray(scene.camera_pose(3, radius=2.0), np.float32)
    intr = (80.0, 80.0, 24.0, 24.0)
    img, mask, _ = model.render_mesh(m, c2w, intr, 48, 48, map='normal_map')
    tex_img, _, _ = model.render_mesh(m, c2w, intr, 48, 48)
    assert int(mask.sum()) > 50 and not torch.equal(img, tex_img)
    with pytest.raises(ValueError):
        model.render_mesh(plain, c2w, intr, 48, 48, map='normal_map')


def test_validation():
    from customnerf_amd import mesh
    v, f = grid(4)
    gv, gf = cuda(v), cuda(f)
    src = mesh.bake_source(gv, gf)
    assert src.normals is None and src.faces.dtype == torch.int32 and abs(src.diagonal - 32 ** 0.5) < 1e-6
    x, n = torch.zeros(5, 3, device="cuda"), torch.ones(5, 3, device="cuda")
    for args in ((src.bvh, x, n, 1.0), (src, x.cpu(), n, 1.0), (src, x, n.cpu(), 1.0), (src, x[:, :2], n, 1.0), (src, x, n[:4], 1.0),
                 (src, x.ravel(), n, 1.0), (src, x, n, 0.0), (src, x, n, -1.0), (src, x, n, float("nan")), (src, x, n, torch.ones(4, device="cuda")),
                 (src, x, n, torch.ones(5)), (src, x.numpy(force=True), n, 1.0)):
        with pytest.raises(ValueError):
            mesh.project_to_surface(*args)
    r = mesh.project_to_surface(src, x, n, torch.ones(5, device="cuda"), want_stats=True)
    assert set(r) == {'point', 'normal', 'offset', 'face', 'kind', 'stats'}
    assert r['kind'].dtype == torch.uint8 and r['face'].dtype == torch.int32 and tuple(r['point'].shape) == (5, 3)
    e = mesh.project_to_surface(src, x[:0], n[:0], 1.0)
    assert tuple(e['point'].shape) == (0, 3) and tuple(e['kind'].shape) == (0,)
    colour = lambda p, d: torch.ones_like(p)                                      # noqa: E731
    with pytest.raises(ValueError):
        mesh.bake_texture(gv, gf, 64, colour, source=src.bvh)
    with pytest.raises(ValueError):
        mesh.bake_texture(gv, gf, 64, colour, reach=0.5)                          # a reach without a source
    with pytest.raises(ValueError):
        mesh.bake_texture(gv, gf, 64, colour, source=mesh.bake_source(gv, gf[:0]))   # no face to take the default reach from
    uvs, tex, extra = mesh.bake_texture(gv, gf, 64, colour, source=src)           # the default reach: 2 % of the source's diagonal
    assert extra['normal_map'] is None and int(extra['kinds'].sum()) == 16 * 16 * 16 and int(extra['kinds'][0]) == 0
