"""GPU: the topology report and the hole filling (csrc/mesh_holes.hip) against their NumPy restatement (tests/holes_restatement.py) —
every count, the loop lengths, and the filled mesh bit for bit — their edge cases, and end to end through NeRFRenderer.extract_mesh /
save_mesh."""
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
import holes_restatement as H  # noqa: E402
import mc_restatement as R  # noqa: E402
import qem_restatement as Q  # noqa: E402
from glb_testlib import parse_glb, read_accessor  # noqa: E402
from mesh_testlib import R_SPHERE, cuda, dtype_guard, gaussian_model, host, octahedron_sphere  # noqa: E402,F401
from holes_testlib import holed_sphere, meshes  # noqa: E402

NAMES = ("cut_sphere", "holed_sphere", "noise", "pinched_sphere", "planar_grid", "sphere", "two_tori")
COUNTS = ("vertices_used", "faces", "edges", "boundary_edges", "nonmanifold_edges", "pinched_vertices", "boundary_loops", "simple_loops",
          "components", "euler", "degenerate_faces", "watertight")
NO_INFO = {"filled": 0, "skipped_pinched": 0, "skipped_long": 0, "new_vertices": 0, "new_faces": 0}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(verts, faces, normals, restated topology, restated fill with normals); computed once, never changed"""
    v, f, n = meshes()[name]
    if n is None:                                                               # every mesh is also filled with normals: any will do
        n = np.tile(np.float32([0.0, 0.6, 0.8]), (len(v), 1))
    return v, f, n, H.topology(v, f), H.fill_holes(v, f, n)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_topology(t, want):
    for k in COUNTS:
        assert t[k] == want[k] and type(t[k]) in (int, bool), k
    ll = t["loop_lengths"]
    assert ll.is_cuda and ll.dtype == torch.int32 and host(ll).tolist() == want["loop_lengths"].tolist()


@pytest.mark.parametrize("name", NAMES)
def test_topology_equals_restatement(name):
    from customnerf_amd import mesh
    v, f, _, want, _ = reference(name)
    t = mesh.topology(cuda(v), cuda(f))
    same_topology(t, want)
    assert set(t) == set(COUNTS) | {"loop_lengths"}


@pytest.mark.parametrize("name", NAMES)
def test_fill_equals_restatement_bit_for_bit(name):
    from customnerf_amd import mesh
    v, f, n, before, (rv, rf, rn, rinfo) = reference(name)
    vo, fo, no, info = mesh.fill_holes(cuda(v), cuda(f), cuda(n))
    assert info == rinfo and all(type(x) is int for x in info.values())
    assert vo.dtype == torch.float32 and fo.dtype == torch.int32 and no.dtype == torch.float32
    assert np.array_equal(host(fo), rf) and np.array_equal(bits(host(vo)), bits(rv)) and np.array_equal(bits(host(no)), bits(rn))
    v2, f2, n2, info2 = mesh.fill_holes(cuda(v), cuda(f))                      # without normals: the same mesh
    assert n2 is None and info2 == rinfo and torch.equal(v2, vo) and torch.equal(f2, fo)
    v3, f3, n3, _ = mesh.fill_holes(cuda(v), cuda(f), cuda(n))                 # and the same bits from a second call
    assert torch.equal(v3, vo) and torch.equal(f3, fo) and torch.equal(n3.view(torch.int32), no.view(torch.int32))
    same_topology(mesh.topology(vo, fo), H.topology(rv, rf))                   # the filled mesh, reported
    if before["boundary_loops"] == 0 or name == "pinched_sphere":               # closed, or nothing simple: equal to the input
        assert np.array_equal(host(fo), f) and np.array_equal(bits(host(vo)), bits(v)) and np.array_equal(bits(host(no)), bits(n))
        assert info == {**NO_INFO, "skipped_pinched": 1 if name == "pinched_sphere" else 0}


def test_max_edges_on_the_cut_sphere():
    from customnerf_amd import mesh
    v, f, n, _, (rv, rf, rn, rinfo) = reference("cut_sphere")
    vo, fo, no, info = mesh.fill_holes(cuda(v), cuda(f), cuda(n), max_edges=63)
    assert info == {**NO_INFO, "skipped_long": 1}
    assert np.array_equal(host(fo), f) and np.array_equal(bits(host(vo)), bits(v)) and np.array_equal(bits(host(no)), bits(n))
    vo, fo, no, info = mesh.fill_holes(cuda(v), cuda(f), cuda(n), max_edges=64)
    assert info == rinfo == {**NO_INFO, "filled": 1, "new_vertices": 1, "new_faces": 64}
    assert np.array_equal(host(fo), rf) and np.array_equal(bits(host(vo)), bits(rv)) and np.array_equal(bits(host(no)), bits(rn))
    assert mesh.topology(vo, fo)["watertight"]


def test_three_loops_alone():
    from customnerf_amd import mesh
    v, f, removed = holed_sphere()
    rv, rf, _, rinfo = H.fill_holes(v, f, None, max_edges=3)
    vo, fo, _, info = mesh.fill_holes(cuda(v), cuda(f), max_edges=3)
    assert info == rinfo == {**NO_INFO, "filled": 1, "skipped_long": 2, "new_faces": 1}
    assert np.array_equal(host(fo), rf) and np.array_equal(bits(host(vo)), bits(v))
    assert tuple(host(fo)[-1]) in {tuple(np.roll(removed, s)) for s in range(3)}


@pytest.mark.parametrize("name", ["noise", "cut_sphere"])
def test_decimate_accepts_the_filled_mesh(name):
    """the patches are edge-manifold and wound like the surface: decimate, the strictest consumer, raises on anything else"""
    from customnerf_amd import mesh
    v, f, n, _, (rv, rf, _, _) = reference(name)
    vo, fo, no, _ = mesh.fill_holes(cuda(v), cuda(f), cuda(n))
    vd, fd, _, _ = mesh.decimate(vo, fo, len(rf) // 2, normals=no)
    assert Q.check_manifold(host(fd)) == 0 and fd.shape[0] < len(rf)
    assert Q.euler(host(fd)) == Q.euler(rf)


def test_bad_meshes_raise_and_empty_meshes_pass():
    from customnerf_amd import mesh
    v, f = octahedron_sphere(1)
    out = f.copy()
    out[2, 1] = len(v)
    neg = f.copy()
    neg[0, 0] = -1
    for bad in (out, neg):
        with pytest.raises(ValueError):
            mesh.topology(cuda(v), cuda(bad))
        with pytest.raises(ValueError):
            mesh.fill_holes(cuda(v), cuda(bad))
    fan = np.concatenate([f, [[f[0, 0], f[0, 1], len(v)]]]).astype(np.int32)     # a third face on one edge
    v3 = np.concatenate([v, [[2.0, 2.0, 2.0]]]).astype(np.float32)
    rep = f.copy()
    rep[3, 2] = rep[3, 0]                                                        # a repeated index
    flip = f.copy()
    flip[5] = flip[5, ::-1]                                                      # a face wound the other way
    for vv, ff in ((v3, fan), (v, rep), (v, flip)):
        same_topology(mesh.topology(cuda(vv), cuda(ff)), H.topology(vv, ff))     # reported ...
        with pytest.raises(ValueError):
            mesh.fill_holes(cuda(vv), cuda(ff))                                  # ... and refused
    ev, ef = torch.zeros(5, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    t = mesh.topology(ev, ef)
    assert t["faces"] == 0 and t["vertices_used"] == 0 and not t["watertight"] and t["loop_lengths"].numel() == 0 and t["euler"] == 0
    vo, fo, no, info = mesh.fill_holes(ev, ef)
    assert torch.equal(vo, ev) and fo.shape == (0, 3) and no is None and info == NO_INFO


def test_tsdf_mesh_filmed_from_above():
    """A sphere fused from the cameras above it only: the face rule leaves a ragged rim where the views end.  Whatever that rim is made
    of — simple loops, pinched vertices — the report and the filled mesh equal the restatement's, and every loop is filled or counted."""
    import tsdf_restatement as T
    from customnerf_amd import mesh
    cams = np.stack([c for c in T.sphere_cameras() if c[2, 3] > 0.1])
    assert 3 <= len(cams) < len(T.sphere_cameras())
    tv = mesh.TSDFVolume(T.SHAPE, T.ORIGIN, T.SPACING, T.TRUNC)
    tv.integrate(cuda(np.stack([T.sphere_depth(c, 'ray') for c in cams])), cams, T.INTRINSICS, depth_kind='ray')
    v, f, n, _ = tv.extract()
    hv, hf, hn = host(v), host(f), host(n)
    want = H.topology(hv, hf)
    t = mesh.topology(v, f)
    same_topology(t, want)
    print(f"filmed from above: {len(hf)} faces, {t['boundary_edges']} boundary edges in {t['boundary_loops']} loops "
          f"{host(t['loop_lengths']).tolist()}, {t['simple_loops']} simple, {t['pinched_vertices']} pinched vertices")
    assert t['boundary_loops'] >= 1 and t['nonmanifold_edges'] == 0 and not t['watertight']
    rv, rf, rn, rinfo = H.fill_holes(hv, hf, hn)
    vo, fo, no, info = mesh.fill_holes(v, f, n)
    assert info == rinfo and info['filled'] + info['skipped_pinched'] == t['boundary_loops']
    assert np.array_equal(host(fo), rf) and np.array_equal(bits(host(vo)), bits(rv)) and np.array_equal(bits(host(no)), bits(rn))
    after = mesh.topology(vo, fo)
    same_topology(after, H.topology(rv, rf))
    assert after['boundary_loops'] == info['skipped_pinched'] and after['watertight'] == (info['skipped_pinched'] == 0)
    assert after['euler'] == t['euler'] + info['filled']


def test_extract_mesh_tsdf_fill(dtype_guard):
    """extract_mesh(tsdf=..., fill_holes=True): the blob rendered from above only, its open underside closed loop by loop"""
    import tsdf_restatement as T
    from customnerf_amd import mesh
    from mesh_testlib import AABB
    model = gaussian_model(dtype_guard, False)
    with torch.no_grad():
        model.aabb_infer.copy_(torch.tensor(AABB))                               # rays start at the box the mesh is taken from
    cams = np.stack([c for c in T.sphere_cameras() if c[2, 3] > 0.1])
    kw = dict(resolution=T.RES, aabb=AABB, topology=True, tsdf=dict(poses=cams, intrinsics=T.INTRINSICS, H=T.IMG, W=T.IMG, min_opacity=0.9))
    a, b = model.extract_mesh(**kw), model.extract_mesh(fill_holes=True, **kw)
    ta, tb, info = a['topology'], b['topology'], b['holes']
    print(f"tsdf from above: {ta['faces']} faces, loops {host(ta['loop_lengths']).tolist()}, {ta['simple_loops']} simple; filled: {info}")
    assert ta['boundary_loops'] >= 1 and not ta['watertight'] and 'holes' not in a and 'tsdf' in b
    assert info['filled'] == ta['simple_loops'] >= 1 and info['skipped_pinched'] == ta['boundary_loops'] - ta['simple_loops']
    assert tb['boundary_loops'] == info['skipped_pinched'] and tb['euler'] == ta['euler'] + info['filled']
    v2, f2, n2, info2 = mesh.fill_holes(a['verts'], a['faces'], a['normals'])
    assert info2 == info and torch.equal(b['verts'], v2) and torch.equal(b['faces'], f2) and torch.equal(b['normals'], n2)


def test_extract_mesh_fills_the_cut(dtype_guard, tmp_path):
    from customnerf_amd import mesh
    model = gaussian_model(dtype_guard, False)
    box = [-0.5, -0.5, -0.5 * R_SPHERE, 0.5, 0.5, 0.5]                          # the box floor cuts the sphere
    kw = dict(resolution=32, threshold=10.0, aabb=box, topology=True)
    cut = model.extract_mesh(**kw)
    t = cut['topology']
    assert not t['watertight'] and t['boundary_loops'] == 1 and t['simple_loops'] == 1 and 'holes' not in cut
    assert 'topology' not in model.extract_mesh(resolution=32, threshold=10.0, aabb=box)
    n_rim = int(t['loop_lengths'][0])
    m = model.extract_mesh(fill_holes=True, **kw)
    assert m['topology']['watertight'] and m['topology']['euler'] == 2 and m['topology']['components'] == 1
    assert m['holes'] == {**NO_INFO, "filled": 1, "new_vertices": 1, "new_faces": n_rim}
    v2, f2, n2, _ = mesh.fill_holes(cut['verts'], cut['faces'], cut['normals'])
    assert torch.equal(m['verts'], v2) and torch.equal(m['faces'], f2) and torch.equal(m['normals'], n2)
    assert model.extract_mesh(fill_holes=n_rim - 1, **kw)['holes'] == {**NO_INFO, "skipped_long": 1}
    for extra in (dict(sparse=True), dict(smooth=5, target_faces=f2.shape[0] // 2)):
        s = model.extract_mesh(fill_holes=True, **extra, **kw)
        assert s['topology']['watertight'] and s['topology']['euler'] == 2, extra
    assert s['faces'].shape[0] in (f2.shape[0] // 2, f2.shape[0] // 2 - 1)
    with pytest.raises(ValueError):
        model.extract_mesh(fill_holes=True, simplify=2, **kw)
    p = str(tmp_path / "closed.ply")
    w = model.save_mesh(p, fill_holes=True, **kw)
    back = R.read_ply(p)
    assert np.array_equal(back["verts"], host(v2)) and np.array_equal(back["faces"], host(f2)) and w['topology']['watertight']
    g = str(tmp_path / "closed.glb")
    model.save_mesh(g, fill_holes=True, **kw)
    doc, blob = parse_glb(g)
    prim, = doc["meshes"][0]["primitives"]
    assert read_accessor(doc, blob, prim["indices"]).reshape(-1, 3).tolist() == host(f2).tolist()
    assert read_accessor(doc, blob, prim["attributes"]["POSITION"]).tobytes() == host(v2).tobytes()
