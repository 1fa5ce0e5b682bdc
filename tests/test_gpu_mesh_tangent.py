"""GPU: the welded vertices and tangent frames (csrc/mesh_tangent.hip) and the tangent-space code of the shared bake (k_bake_tspace of
csrc/mesh_bake.h) against their NumPy restatement (tests/tangent_restatement.py), integers exact and floats bit for bit, and the layers
above them: bake_texture(normal_map='tangent'), extract_mesh(normal_map='tangent'), save_mesh to a .glb path, with what existed before
(normal_map=True, OBJ) unchanged."""
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
import tangent_restatement as TR  # noqa: E402
import tangent_testlib as TL  # noqa: E402
from glb_testlib import image_bytes, parse_glb, read_accessor, read_png_bytes  # noqa: E402
from mesh_testlib import AABB, cuda, dtype_guard, gaussian_model  # noqa: E402,F401

F32 = np.float32
SENTINEL = -7.0
PAD = 8
GUARD = 256


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def gpu_passes(v, f, uv, n):
    """cnerf_mesh_tangent_weld / _frames / _vertices into sentinel-padded buffers, with a workspace of exactly the queried size and a guard
    band behind it -> dict of arrays without the (checked) padding"""
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib, check, ptr, stream
    V, F = len(v), len(f)
    p = lambda t: ptr(t) if t is not None and t.numel() else None                # noqa: E731
    gv, gf, guv = cuda(np.asarray(v, F32).reshape(-1, 3)), cuda(np.asarray(f, np.int32).reshape(-1, 3)), cuda(np.asarray(uv, F32))
    gn = None if n is None else cuda(np.asarray(n, F32))
    nbytes = mesh.tangent_workspace_bytes(V, F)
    ws = torch.full((nbytes + GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    ints = lambda k: torch.full((k + PAD,), int(SENTINEL), dtype=torch.int32, device="cuda")     # noqa: E731
    floats = lambda k: torch.full((k + PAD,), SENTINEL, device="cuda")         # noqa: E731
    counts, cv, vc, tan = ints(2), ints(3 * F), ints(3 * F), floats(12 * F)
    check(lib.cnerf_mesh_tangent_weld(p(gf), p(guv), V, F, ptr(ws), nbytes, ptr(counts), ptr(cv), F, ptr(vc), 3 * F, stream()), "weld")
    W, flags = (int(c) for c in counts[:2].cpu())
    out = {'W': W, 'flags': flags}
    check(lib.cnerf_mesh_tangent_frames(p(gv), p(gf), p(guv), p(gn), V, F, ptr(ws), nbytes, ptr(tan), F, stream()), "frames")
    pos, nrm, uvo, tano, idx = floats(3 * W), floats(3 * W), floats(2 * W), floats(4 * W), ints(3 * F)
    check(lib.cnerf_mesh_tangent_vertices(p(gv), p(gf), p(guv), p(gn), ptr(tan), ptr(cv), ptr(vc), V, F, W, ptr(ws), nbytes, ptr(pos), ptr(nrm),
                                          ptr(uvo), ptr(tano), ptr(idx), stream()), "vertices")
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0x5a).all()                                          # nothing written past the queried size
    wrote = flags == 0
    for name, t, k, shape in (('corner_vertex', cv, 3 * F, (F, 3)), ('vertex_corner', vc, W, (W,)), ('tangents', tan, 12 * F, (F, 3, 4)),
                              ('positions', pos, 3 * W, (W, 3)), ('normals', nrm, 3 * W, (W, 3)), ('uvs', uvo, 2 * W, (W, 2)),
                              ('tangents_w', tano, 4 * W, (W, 4)), ('indices', idx, 3 * F, (F, 3))):
        a = t.cpu().numpy()
        assert (a[k:] == a.dtype.type(SENTINEL)).all(), name
        if not wrote:
            assert (a == a.dtype.type(SENTINEL)).all(), name                    # after a bad index nothing is written
        out[name] = a[:k].reshape(shape)
    assert (counts[2:].cpu().numpy() == int(SENTINEL)).all()
    return out


def check_against_restatement(v, f, uv, n):
    from customnerf_amd import mesh
    got = gpu_passes(v, f, uv, n)
    want_t, want_gn, cv, vc = TR.frames(v, f, uv, n)
    want = TR.vertices(v, f, uv, n)
    assert got['flags'] == 0 and got['W'] == len(vc)
    assert got['corner_vertex'].tolist() == cv.tolist() and got['vertex_corner'].tolist() == vc.tolist()
    assert same_bits(got['tangents'], want_t)
    assert got['indices'].tolist() == cv.tolist()
    for k, g in (('positions', 'positions'), ('normals', 'normals'), ('uvs', 'uvs'), ('tangents', 'tangents_w')):
        assert same_bits(got[g], want[k]), k
    # the public functions give the same arrays
    gv, gf, guv = cuda(np.asarray(v, F32)), cuda(np.asarray(f, np.int32)), cuda(np.asarray(uv, F32))
    gn = None if n is None else cuda(np.asarray(n, F32))
    a, b = mesh.weld_corners(gf, guv, V=len(v))
    assert a.dtype == torch.int32 and b.dtype == torch.int32 and a.cpu().tolist() == cv.tolist() and b.cpu().tolist() == vc.tolist()
    assert same_bits(mesh.corner_tangents(gv, gf, guv, gn).cpu().numpy(), want_t)
    g = mesh.gltf_vertices(gv, gf, guv, gn)
    assert sorted(g) == ['indices', 'normals', 'positions', 'tangents', 'uvs']
    for k in ('positions', 'normals', 'uvs', 'tangents'):
        assert g[k].dtype == torch.float32 and same_bits(g[k].cpu().numpy(), want[k]), k
    assert g['indices'].dtype == torch.uint32 and tuple(g['indices'].shape) == (len(f), 3)
    assert g['indices'].cpu().numpy().tolist() == cv.tolist()
    return got


@pytest.mark.parametrize("with_normals", [True, False])
def test_hand_soup(with_normals):
    v, f, uv, n, names = TL.hand_soup()
    got = check_against_restatement(v, f, uv, n if with_normals else None)
    assert got['W'] == 20
    np.testing.assert_array_equal(got['tangents'][names["quad"], 0], np.array([1, 0, 0, 1], F32))
    np.testing.assert_array_equal(got['tangents'][names["mirrored"], 0], np.array([-1, 0, 0, -1], F32))


@pytest.mark.parametrize("layout,with_normals", [("uniform", True), ("area", True), ("area", False)])
def test_icosphere(layout, with_normals):
    """the 80-face icosphere with the UVs of the uniform and the area layout at R = 64"""
    s = L.sphere()
    v, f = s['lv'], s['lf']
    assert len(f) == 80
    uv, _ = TL.layout_uvs(layout, v, f, 64)
    got = check_against_restatement(v, f, uv, v if with_normals else None)
    assert got['W'] == 240                                                      # every face has a cell of its own: no corner is shared


@pytest.mark.parametrize("with_normals", [True, False])
def test_golden_sphere_projected(with_normals):
    v, f, n = TL.decimated_sphere()
    uv, _ = TL.layout_uvs('projected', v, f, 64, n)
    got = check_against_restatement(v, f, uv, n if with_normals else None)
    assert got['W'] == 219


def test_empty_and_single_face():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], F32)
    for f, uv in ((np.zeros((0, 3), np.int32), np.zeros((0, 3, 2), F32)),
                  (np.array([[0, 1, 2]], np.int32), np.array([[[0.1, 0.1], [0.9, 0.1], [0.1, 0.9]]], F32))):
        for n in (None, np.tile(np.array([0, 0, 1], F32), (4, 1))):
            got = check_against_restatement(v, f, uv, n)
            assert got['W'] == 3 * len(f)
    got = gpu_passes(np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), np.zeros((0, 3, 2), F32), None)
    assert got['W'] == 0 and got['flags'] == 0


@pytest.mark.parametrize("bad", [-1, 152])
def test_bad_index(bad):
    from customnerf_amd import mesh
    v, f, n = TL.decimated_sphere()
    uv, _ = TL.layout_uvs('uniform', v, f, 64)
    f = f.copy()
    f[137, 1] = bad
    got = gpu_passes(v, f, uv, n)                                               # checks that no output was written
    assert got['flags'] == 1 and got['W'] == 0
    gv, gf, guv = cuda(v), cuda(f), cuda(uv)
    for call in (lambda: mesh.weld_corners(gf, guv, V=len(v)), lambda: mesh.corner_tangents(gv, gf, guv), lambda: mesh.gltf_vertices(gv, gf, guv)):
        with pytest.raises(ValueError, match="index"):
            call()


# ---------------------------------------------------------------------------------------------------------------- the per-texel code
def make_layout(layout, gv, gf, gn, R):
    from customnerf_amd import mesh
    return mesh._LAYOUTS[layout](gv, gf, gn, R, "test", 2)


def texel_table(layout, v, f, n, R):
    uv, plan = TL.layout_uvs(layout, v, f, R, n)
    return uv, TR.texels(layout, plan, v, f, R, n)


@pytest.mark.parametrize("layout", ["uniform", "area", "projected"])
def test_tspace_matches_restatement(layout):
    """the code of given normals on the 80-face icosphere at R = 64: floats bit for bit, the stored map byte for byte; one call over
    [0, total) equals three ragged calls; without m the code is (0.5, 0.5, 1)"""
    from customnerf_amd import mesh
    s = L.sphere()
    v, f, n, R = s['lv'], s['lf'], s['lv'], 64
    uv, (face, w1, w2, corner, flat, N, X, Y) = texel_table(layout, v, f, n, R)
    tan = TR.frames(v, f, uv, n)[0]
    total = len(face)
    rng = np.random.default_rng(7)
    m = (N + 0.4 * rng.standard_normal(N.shape)).astype(F32)
    m = (m / np.linalg.norm(m, axis=1, keepdims=True)).astype(F32)
    m[::97] = 0                                                                 # a zero normal: the grey code (0.5, 0.5, 0.5)
    want = TR.tspace(tan, face, w1, w2, corner, flat, N, m)
    gv, gf, gn = cuda(v), cuda(f), cuda(n)
    lay = make_layout(layout, gv, gf, gn, R)
    assert lay.total == total and same_bits(lay.uvs.cpu().numpy(), uv)
    gt = mesh.corner_tangents(gv, gf, lay.uvs, gn)
    assert same_bits(gt.cpu().numpy(), tan)
    gm = torch.full((total, 4), SENTINEL, device="cuda")                        # a row stride of 4
    gm[:, :3] = cuda(m)
    out = torch.full((total + PAD, 3), SENTINEL, device="cuda")
    lay.tspace(0, total, gt, gm, out)
    got = out.cpu().numpy()
    assert (got[total:] == SENTINEL).all()
    assert same_bits(got[:total], want)
    cuts = [0, total // 3 + 1, total // 3 + 2, total]                           # three ragged calls, one of a single texel
    parts = torch.full((total, 3), SENTINEL, device="cuda")
    for a, b in zip(cuts[:-1], cuts[1:]):
        lay.tspace(a, b, gt, gm[a:b], parts[a:b])
    assert torch.equal(parts, out[:total])
    # through the existing fill and store: the map, byte for byte
    fill = (mesh.C.c_uint8 * 3)(128, 128, 255)
    img = torch.zeros(R, R, 3, dtype=torch.uint8, device="cuda")
    lay.fill(img, fill)
    lay.store(0, total, out[:total], fill, img)
    want_map = np.full((R, R, 3), (128, 128, 255), np.uint8)
    own = face >= 0
    want_map[Y[own], X[own]] = TR.store_u8(want)[own]
    np.testing.assert_array_equal(img.cpu().numpy(), want_map)
    assert len(np.unique(want_map[Y[own], X[own]], axis=0)) > 100               # a map with content
    lay.tspace(0, total, gt, None, out)
    assert (out[:total].cpu().numpy() == np.array([0.5, 0.5, 1.0], F32)).all()


def grey(x, d):
    return torch.full((x.shape[0], 3), 0.25, device=x.device)


@pytest.mark.parametrize("layout", ["uniform", "area", "projected"])
def test_bake_without_source_is_flat(layout):
    """bake_texture(normal_map='tangent') without a source encodes the mesh's own normal: every owned texel is exactly (128, 128, 255),
    and so are the texels nobody owns, by the fill"""
    from customnerf_amd import mesh
    v, f, n = TL.decimated_sphere()
    gv, gf, gn = cuda(v), cuda(f), cuda(n)
    uvs, tex, extra = mesh.bake_texture(gv, gf, 64, grey, normals=gn, layout=layout, normal_map='tangent', chunk=777)
    nm = extra['normal_map'].cpu().numpy()
    assert nm.shape == (64, 64, 3) and nm.dtype == np.uint8 and (nm == np.array([128, 128, 255], np.uint8)).all()
    assert extra['normal_space'] == 'tangent' and extra['kinds'].cpu().tolist() == [0, 0, 0, 0]
    assert same_bits(extra['tangents'].cpu().numpy(), TR.frames(v, f, uvs.cpu().numpy(), n)[0])
    plain = mesh.bake_texture(gv, gf, 64, grey, normals=gn, layout=layout)
    assert len(plain) == 2 and torch.equal(plain[0], uvs) and torch.equal(plain[1], tex)
    _, tex2, extra2 = mesh.bake_texture(gv, gf, 64, grey, normals=gn, layout=layout, normal_map=True)
    assert extra2['normal_space'] == 'object' and 'tangents' not in extra2 and torch.equal(tex2, tex)
    owned = (tex.cpu().numpy() != 0).any(2)
    assert 0 < owned.sum() < 64 * 64 and (extra2['normal_map'].cpu().numpy()[~owned] == 128).all()
    with pytest.raises(ValueError, match="normal_map"):
        mesh.bake_texture(gv, gf, 64, grey, normals=gn, normal_map='object')


@pytest.mark.parametrize("layout", ["uniform", "area", "projected"])
def test_tangent_map_agrees_with_object_map(layout):
    """With source= the 1280-face icosphere and the mesh its decimation to 200 faces: every owned texel of the tangent-space map, decoded
    with the frame the restatement gives that texel, points where the object-space map (normal_map=True) points at the same texel, to
    within 1 degree.  Each map's 8-bit quantisation moves its vector by at most sqrt(3) / 255, so two unit vectors differ by at most
    2 sqrt(3) / 255 rad = 0.78 degrees; the rest is slack for float32 and the renormalisation: a derived figure, not a measured one.
    Left out are only texels whose object-space byte triple decodes to a vector shorter than 0.5 (on this input: none)."""
    from customnerf_amd import mesh
    s = L.sphere()
    sv, sf = cuda(s['sv']), cuda(s['sf'])
    gv, gf, gn, _ = mesh.decimate(sv, sf, 200, normals=sv)
    v, f, n = gv.cpu().numpy(), gf.cpu().numpy(), gn.cpu().numpy()
    assert 80 <= len(f) <= 300
    src = mesh.bake_source(sv, sf, sv)
    R = 64
    kw = dict(normals=gn, layout=layout, source=src, reach=0.25)
    uvs, tex, et = mesh.bake_texture(gv, gf, R, grey, normal_map='tangent', **kw)
    uvs_o, tex_o, eo = mesh.bake_texture(gv, gf, R, grey, normal_map=True, **kw)
    assert torch.equal(uvs, uvs_o) and torch.equal(tex, tex_o) and torch.equal(et['kinds'], eo['kinds'])
    uv, (face, w1, w2, corner, flat, N, X, Y) = texel_table(layout, v, f, n, R)
    assert same_bits(uvs.cpu().numpy(), uv)
    tan = TR.frames(v, f, uv, n)[0]
    assert same_bits(et['tangents'].cpu().numpy(), tan)
    own = face >= 0
    face, w1, w2, corner, flat, N, X, Y = (a[own] for a in (face, w1, w2, corner, flat, N, X, Y))
    t, B = TR.texel_frames(tan, face, w1, w2, corner, flat, N)
    tmap, omap = et['normal_map'].cpu().numpy(), eo['normal_map'].cpu().numpy()
    a = TR.decode(tmap[Y, X], t, B, N)
    b = omap[Y, X].astype(np.float64) / 255.0 * 2.0 - 1.0
    keep = np.linalg.norm(b, axis=1) >= 0.5                                     # the cap: shorter object-space vectors carry no direction
    assert keep.all()
    cos = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    angle = np.degrees(np.arccos(np.clip(cos[keep], -1, 1)))
    tilt = np.degrees(np.arccos(np.clip((b / np.linalg.norm(b, axis=1, keepdims=True) * N).sum(1), -1, 1)))
    print(f"{layout}: {len(face)} owned texels of {len(f)} faces, tangent vs object map: max {angle.max():.3f} deg, mean {angle.mean():.3f} deg; "
          f"the source's normal tilts up to {tilt.max():.1f} deg from the mesh's")
    assert angle.max() <= 1.0
    assert tilt.max() > 3.0                                                     # the map holds detail the mesh lost: not a flat map
    un = np.ones((R, R), bool)
    un[Y, X] = False
    assert (tmap[un] == np.array([128, 128, 255], np.uint8)).all()


# ---------------------------------------------------------------------------------------------------------------- through the renderer
def test_extract_and_save_glb(dtype_guard, tmp_path):
    """extract_mesh(normal_map='tangent') on a small field, save_mesh to .glb parsed back against gltf_vertices of the returned dict and
    its two images, textureless .glb files with colours and with AO, and the refused combinations"""
    from customnerf_amd import mesh
    model = gaussian_model(dtype_guard, False)
    kw = dict(resolution=32, threshold=10.0, aabb=AABB)
    low = dict(target_faces=200, texture=64, bake_from='source', **kw)
    path = str(tmp_path / "m.glb")
    m = model.save_mesh(path, normal_map='tangent', **low)
    F, V = m['faces'].shape[0], m['verts'].shape[0]
    assert 0 < F <= 200
    assert m['normal_space'] == 'tangent'
    assert tuple(m['normal_map'].shape) == (64, 64, 3) and m['normal_map'].dtype == torch.uint8
    assert tuple(m['tangents'].shape) == (F, 3, 4) and m['tangents'].dtype == torch.float32
    assert tuple(m['uvs'].shape) == (F, 3, 2) and tuple(m['texture'].shape) == (64, 64, 3) and tuple(m['bake_kinds'].shape) == (4,)
    nm = m['normal_map'].cpu().numpy()
    assert (nm[..., 2] >= 128).all() and len(np.unique(nm.reshape(-1, 3), axis=0)) > 50          # a map with content, pointing outwards
    want_t = TR.frames(m['verts'].cpu().numpy(), m['faces'].cpu().numpy(), m['uvs'].cpu().numpy(), m['normals'].cpu().numpy())[0]
    assert same_bits(m['tangents'].cpu().numpy(), want_t)
    g = mesh.gltf_vertices(m['verts'], m['faces'], m['uvs'], m['normals'])
    doc, blob = parse_glb(path)
    prim, = doc["meshes"][0]["primitives"]
    att = prim["attributes"]
    assert set(att) == {"POSITION", "NORMAL", "TEXCOORD_0", "TANGENT"}
    assert read_accessor(doc, blob, prim["indices"]).tobytes() == g['indices'].cpu().numpy().astype("<u4").tobytes()
    for key, name in (("POSITION", 'positions'), ("NORMAL", 'normals'), ("TEXCOORD_0", 'uvs'), ("TANGENT", 'tangents')):
        assert read_accessor(doc, blob, att[key]).tobytes() == g[name].cpu().numpy().tobytes(), key
    mat, = doc["materials"]
    t_img = doc["textures"][mat["pbrMetallicRoughness"]["baseColorTexture"]["index"]]["source"]
    n_img = doc["textures"][mat["normalTexture"]["index"]]["source"]
    np.testing.assert_array_equal(read_png_bytes(image_bytes(doc, blob, t_img)), m['texture'].cpu().numpy())
    np.testing.assert_array_equal(read_png_bytes(image_bytes(doc, blob, n_img)), nm)
    assert "extensionsUsed" not in doc                                          # lit: it carries a normal map
    # without bake_from='source' the map is flat
    flat = model.extract_mesh(normal_map='tangent', target_faces=200, texture=64, **kw)
    assert (flat['normal_map'].cpu().numpy() == np.array([128, 128, 255], np.uint8)).all() and 'bake_kinds' not in flat
    # textureless: the indexed mesh with its colours, or with the AO as grey
    for name, opts in (("c.glb", dict(color=True)), ("a.glb", dict(ao=8))):
        p2 = str(tmp_path / name)
        c = model.save_mesh(p2, target_faces=200, **opts, **kw)
        doc, blob = parse_glb(p2)
        prim, = doc["meshes"][0]["primitives"]
        att = prim["attributes"]
        assert set(att) == {"POSITION", "NORMAL", "COLOR_0"} and "images" not in doc and doc["extensionsUsed"] == ["KHR_materials_unlit"]
        assert read_accessor(doc, blob, att["POSITION"]).tobytes() == c['verts'].cpu().numpy().tobytes()
        assert read_accessor(doc, blob, att["NORMAL"]).tobytes() == c['normals'].cpu().numpy().tobytes()
        assert read_accessor(doc, blob, prim["indices"]).tobytes() == c['faces'].cpu().numpy().astype("<u4").tobytes()
        col = c['colors'].cpu().numpy() if 'ao' not in c else np.repeat((c['ao'] * 255).round().to(torch.uint8).cpu().numpy()[:, None], 3, 1)
        rgba = read_accessor(doc, blob, att["COLOR_0"])
        assert col.shape == (c['verts'].shape[0], 3) and (rgba[:, :3] == col).all() and (rgba[:, 3] == 255).all()
    # the refused combinations, before anything is extracted or written
    for name, opts in (("r.glb", dict(normal_map=True, texture=64)), ("r.obj", dict(normal_map='tangent', texture=64)),
                       ("r.ply", dict(normal_map='tangent', texture=64)), ("r.ply", dict(normal_map=True, texture=64)),
                       ("r.ply", dict(normal_map='tangent')), ("r.ply", dict(normal_map=True))):
        with pytest.raises(ValueError):
            model.save_mesh(str(tmp_path / name), **opts, **kw)
        assert not os.path.exists(str(tmp_path / name))
    with pytest.raises(ValueError):
        model.extract_mesh(normal_map='tangent', **kw)                          # no atlas to share
    with pytest.raises(ValueError):
        model.extract_mesh(normal_map='object', texture=64, **kw)


def test_object_space_and_obj_unchanged(dtype_guard, tmp_path):
    """extract_mesh(normal_map=True) and save_mesh to .obj give what they gave: the map is the restatement of the projection
    (tests/project_restatement.py) through the store's rounding, the files are the OBJ, the material with its `norm` line and both PNGs;
    the only new key is 'normal_space'"""
    model = gaussian_model(dtype_guard, False)
    res = 28
    kw = dict(resolution=res, threshold=10.0, aabb=AABB)
    base = model.extract_mesh(**kw)
    assert 'normal_map' not in base and 'normal_space' not in base and 'tangents' not in base
    path = str(tmp_path / "low.obj")
    m = model.save_mesh(path, bake_from='source', normal_map=True, target_faces=200, texture=64, **kw)
    assert m['normal_space'] == 'object' and 'tangents' not in m
    F = m['faces'].shape[0]
    v, f, n = m['verts'].cpu().numpy(), m['faces'].cpu().numpy(), m['normals'].cpu().numpy()
    step = F32(1.0) / F32(res - 1)
    x, d = A.points(v, f, 64, normals=n)
    want = P.project(base['verts'].cpu().numpy(), base['faces'].cpu().numpy(), base['normals'].cpu().numpy(), x, -d, F32(4.0) * step)
    face, _, _, X, Y = A.cell_texels(F, 64)
    want_map = np.full((64, 64, 3), 128, np.uint8)
    want_map[Y[face >= 0], X[face >= 0]] = P.normal_texels(want['normal'])[face >= 0]
    np.testing.assert_array_equal(m['normal_map'].cpu().numpy(), want_map)
    assert m['bake_kinds'].cpu().tolist() == P.kinds(want['kind']).tolist()
    assert same_bits(m['uvs'].cpu().numpy(), A.uvs(F, 64))
    np.testing.assert_array_equal(A.read_png(str(tmp_path / "low_normal.png")), want_map)
    np.testing.assert_array_equal(A.read_png(str(tmp_path / "low.png")), m['texture'].cpu().numpy())
    assert open(str(tmp_path / "low.mtl")).read() == "newmtl material0\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd low.png\nnorm low_normal.png\n"
    o = A.read_obj(path)
    assert same_bits(o['verts'], v) and same_bits(o['uvs'], A.uvs(F, 64).reshape(-1, 2)) and same_bits(o['normals'], n)
    assert (o['f'][..., 0] - 1).tolist() == f.tolist() and o['mtllib'] == "low.mtl"
    assert sorted(os.listdir(str(tmp_path))) == ["low.mtl", "low.obj", "low.png", "low_normal.png"]
