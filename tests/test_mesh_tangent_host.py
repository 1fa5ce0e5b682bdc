"""CPU: the rules of the welded vertices, tangent frames and tangent-space code (include/customnerf_hip.h, cnerf_mesh_tangent_*) as
tests/tangent_restatement.py states them, on hand cases and on the decimated golden sphere, and the new entry points' argument checks,
which return before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import tangent_restatement as TR  # noqa: E402
import tangent_testlib as TL  # noqa: E402

f32 = np.float32
PASSES = ("cnerf_mesh_tangent_workspace_bytes", "cnerf_mesh_tangent_weld", "cnerf_mesh_tangent_frames", "cnerf_mesh_tangent_vertices",
          "cnerf_mesh_atlas_tspace", "cnerf_mesh_atlas_sized_tspace", "cnerf_mesh_atlas_proj_tspace")


@pytest.fixture(autouse=True)
def passes_exist():
    """the rules restated here are those of entry points the library exports and the binding lists: without them they describe nothing"""
    from customnerf_amd import _lib
    for name in PASSES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name


def test_hand_cases():
    v, f, uv, n, names = TL.hand_soup()
    tan, gn, cv, vc = TR.frames(v, f, uv, n)
    ok, cT, cB, cN, det = TR.face_terms(v, f, uv)
    # the unit quad with identity UVs: t = +x, w = +1; with u mirrored: t = -x (where u grows) and w = -1
    for name, t, w in (("quad", (1, 0, 0), 1), ("quad_b", (1, 0, 0), 1), ("mirrored", (-1, 0, 0), -1), ("mirrored_b", (-1, 0, 0), -1)):
        assert ok[names[name]]
        np.testing.assert_array_equal(tan[names[name]], np.tile(np.array(t + (w,), f32), (3, 1)))
    assert det[names["quad"]] > 0 and det[names["mirrored"]] < 0
    # a face without UV area and a face without area give nothing: the fallback, the axis most orthogonal to the normal
    assert det[names["det_zero"]] == 0 and not ok[names["det_zero"]] and not ok[names["zero_area"]] and det[names["zero_area"]] != 0
    t = tan[names["det_zero"], 0]                                              # n = (0.6, 0, 0.8): the smallest |n_k| is y
    np.testing.assert_array_equal(t, np.array([0, 1, 0, 1], f32))
    t = tan[names["zero_area"], 0]                                             # n = (0, 1, 0): a tie between x and z, the lowest wins
    np.testing.assert_array_equal(t, np.array([1, 0, 0, 1], f32))
    # without normals these groups have no normal either: n = 0, t = (1, 0, 0), w = +1
    tan0, gn0, _, _ = TR.frames(v, f, uv, None)
    for name in ("det_zero", "zero_area"):
        np.testing.assert_array_equal(tan0[names[name]], np.tile(np.array([1, 0, 0, 1], f32), (3, 1)))
        assert (gn0[cv[names[name]]] == 0).all()
    np.testing.assert_array_equal(tan0[names["quad"]], tan[names["quad"]])
    np.testing.assert_array_equal(gn0[cv[names["quad"]]], np.tile(np.array([0, 0, 1], f32), (3, 1)))
    # a vertex on a seam between two charts is two output vertices; the quad's shared corners are one each
    for s in ("seam_a", "seam_b"):
        groups = set(cv.reshape(-1)[f.reshape(-1) == names[s]].tolist())
        assert len(groups) == 2
    assert cv[names["quad"], 0] == cv[names["quad_b"], 0] and cv[names["quad"], 2] == cv[names["quad_b"], 1]
    assert len(vc) == 4 + 4 + 3 + 3 + 6
    # the numbering: ascending vertex, then ascending smallest corner; vertex_corner is the smallest corner of its group
    fv = f.reshape(-1)
    key = [(int(fv[c]), int(c)) for c in vc]
    assert key == sorted(key)
    for w, c in enumerate(vc):
        assert c == np.nonzero(cv.reshape(-1) == w)[0].min()
    g = TR.vertices(v, f, uv, n)
    np.testing.assert_array_equal(g['positions'], v[fv[vc]])
    np.testing.assert_array_equal(g['uvs'], np.stack([uv.reshape(-1, 2)[vc, 0], f32(1) - uv.reshape(-1, 2)[vc, 1]], -1))
    np.testing.assert_array_equal(g['indices'], cv) and g['indices'].dtype == np.uint32
    np.testing.assert_array_equal(g['tangents'], tan.reshape(-1, 4)[vc])


def test_weld_keys_are_bit_patterns():
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    uv = np.zeros((2, 3, 2), f32)
    cv, vc = TR.weld(f, uv)
    assert cv.tolist() == [[0, 1, 2], [0, 2, 3]] and vc.tolist() == [0, 1, 2, 5]
    uv[1, 0, 0] = -0.0                                                         # -0 is not +0
    cv, vc = TR.weld(f, uv)
    assert cv.tolist() == [[0, 2, 3], [1, 3, 4]] and vc.tolist() == [0, 3, 1, 2, 5]


@pytest.mark.parametrize("R", [64, 256])
def test_golden_sphere(R):
    """the decimated sphere under the projected layout: 219 welded vertices of 900 corners, every chart keeps its orientation; the code of
    a normal decodes back to it within the quantisation"""
    v, f, n = TL.decimated_sphere()
    assert v.shape == (152, 3) and f.shape == (300, 3)
    uv, p = TL.layout_uvs('projected', v, f, R, n)
    tan, gn, cv, vc = TR.frames(v, f, uv, n)
    ok, _, _, _, det = TR.face_terms(v, f, uv)
    assert len(vc) == 219 and cv.max() == 218
    assert (det > 0).all() and ok.all()
    assert (tan[..., 3] == 1).all()
    t3 = tan[..., :3].astype(np.float64)
    np.testing.assert_allclose(np.linalg.norm(t3, axis=-1), 1.0, atol=1e-6)
    # every frame is orthogonal to its vertex normal
    nn = n[f].astype(np.float64)
    nn /= np.linalg.norm(nn, axis=-1, keepdims=True)
    assert np.abs((t3 * nn).sum(-1)).max() < 1e-6
    # round trip: the code of m, decoded with the texel's own (t, B, N), is m to within the quantisation (each byte moves its component by
    # at most 1 / 255, the vector by at most sqrt(3) / 255, plus float32 rounding)
    face, w1, w2, corner, flat, N, X, Y = TR.texels('projected', p, v, f, R, n)
    assert (face >= 0).all() and len(face) == p.total
    rng = np.random.default_rng(3)
    m = (N + 0.35 * rng.standard_normal(N.shape)).astype(f32)
    m = (m / np.linalg.norm(m, axis=1, keepdims=True)).astype(f32)
    rgb = TR.tspace(tan, face, w1, w2, corner, flat, N, m)
    assert rgb.dtype == f32 and rgb.min() >= 0 and rgb.max() <= 1
    t, B = TR.texel_frames(tan, face, w1, w2, corner, flat, N)
    back = TR.decode(TR.store_u8(rgb), t, B, N)
    err = np.linalg.norm(back - m.astype(np.float64), axis=1).max()
    print(f"R = {R}: {p.total} texels, round trip error {err:.5f} (allowed {np.sqrt(3) / 255 + 1e-5:.5f})")
    assert err <= np.sqrt(3) / 255 + 1e-5
    # the frame is orthonormal and right-handed for w = +1
    assert np.abs((t.astype(np.float64) * N).sum(1)).max() < 1e-6 and np.abs((B.astype(np.float64) * t).sum(1)).max() < 1e-6
    np.testing.assert_allclose(np.cross(N.astype(np.float64), t.astype(np.float64)), B, atol=1e-6)
    # the mesh's own normal has the code (0.5, 0.5, 1) exactly: the flat map
    flat_map = TR.store_u8(TR.tspace(tan, face, w1, w2, corner, flat, N, None))
    assert (flat_map == np.array([128, 128, 255], np.uint8)).all()


one = ctypes.c_void_p(256)                                                    # non-NULL, 16-byte aligned, never dereferenced on these paths
BIG = 1 << 40


def _weld(lib, **over):
    a = dict(faces=one, uvs=one, V=8, F=4, ws=one, ws_bytes=BIG, counts=one, cv=one, max_faces=4, vc=one, max_verts=12, stream=None)
    a.update(over)
    return lib.cnerf_mesh_tangent_weld(a["faces"], a["uvs"], a["V"], a["F"], a["ws"], a["ws_bytes"], a["counts"], a["cv"], a["max_faces"],
                                       a["vc"], a["max_verts"], a["stream"])


def test_argument_return_codes_without_launch():
    """CNERF_EINVAL (-1) and CNERF_ENULL (-2) of the new entry points, returned before anything touches the device"""
    from customnerf_amd._lib import lib
    need = ctypes.c_uint64(0)
    assert lib.cnerf_mesh_tangent_workspace_bytes(152, 300, ctypes.byref(need)) == 0
    small = need.value
    assert small >= 256 + 4 * 4 * 152 + (4 + 4 + 12) * 900 and small % 256 == 0
    assert lib.cnerf_mesh_tangent_workspace_bytes(0, 0, ctypes.byref(need)) == 0 and need.value >= 256
    assert lib.cnerf_mesh_tangent_workspace_bytes(152, 300, None) == -2
    assert lib.cnerf_mesh_tangent_workspace_bytes(1 << 31, 300, ctypes.byref(need)) == -1
    assert lib.cnerf_mesh_tangent_workspace_bytes(152, 0x2AAAAAAB, ctypes.byref(need)) == -1
    # weld
    assert _weld(lib, V=1 << 31) == -1 and _weld(lib, F=0x2AAAAAAB) == -1
    assert _weld(lib, ws=None) == -2
    assert _weld(lib, V=152, F=300, ws_bytes=small - 1) == -1                   # a short workspace
    assert _weld(lib, ws=ctypes.c_void_p(264)) == -1                            # not 16-byte aligned
    for k in ("faces", "uvs", "counts", "cv", "vc"):
        assert _weld(lib, **{k: None}) == -2, k
    # frames and vertices
    fr = lambda **o: lib.cnerf_mesh_tangent_frames(*[dict(dict(v=one, f=one, uv=one, n=None, V=8, F=4, ws=one, b=BIG, t=one, mf=4, s=None), **o)[k]  # noqa: E731
                                                     for k in ("v", "f", "uv", "n", "V", "F", "ws", "b", "t", "mf", "s")])
    assert fr(V=1 << 31) == -1 and fr(ws=None) == -2 and fr(V=152, F=300, b=small - 1) == -1
    for k in ("v", "f", "uv", "t"):
        assert fr(**{k: None}) == -2, k
    assert fr(F=0) == 0 and fr(mf=0) == 0                                      # nothing to do: no launch
    names = ("v", "f", "uv", "n", "t", "cv", "vc", "V", "F", "W", "ws", "b", "po", "no", "uo", "to", "ix", "s")
    base = dict(v=one, f=one, uv=one, n=None, t=one, cv=one, vc=one, V=8, F=4, W=6, ws=one, b=BIG, po=one, no=one, uo=one, to=one, ix=one, s=None)
    vx = lambda **o: lib.cnerf_mesh_tangent_vertices(*[dict(base, **o)[k] for k in names])  # noqa: E731
    assert vx(W=13) == -1 and vx(F=0x2AAAAAAB) == -1 and vx(ws=None) == -2 and vx(V=152, F=300, b=small - 1) == -1
    for k in ("v", "f", "uv", "t", "cv", "vc", "po", "no", "uo", "to", "ix"):
        assert vx(**{k: None}) == -2, k
    assert vx(F=0, W=0) == 0
    # the per-texel code of the three layouts: the range and the stride first, then the pointers
    uni = lambda **o: lib.cnerf_mesh_atlas_tspace(*[dict(dict(v=one, n=None, V=8, f=one, F=4, R=64, t=one, t0=0, t1=16, m=one, ms=3, fl=one, o=one,  # noqa: E731
                                                              mp=16, s=None), **o)[k]
                                                    for k in ("v", "n", "V", "f", "F", "R", "t", "t0", "t1", "m", "ms", "fl", "o", "mp", "s")])
    assert uni(R=8) == -1 and uni(t0=17) == -1 and uni(t1=2 * 32 * 32 + 1) == -1 and uni(ms=2) == -1 and uni(V=1 << 31) == -1
    for k in ("v", "f", "t", "fl", "o"):
        assert uni(**{k: None}) == -2, k
    assert uni(t1=0) == 0 and uni(mp=0) == 0
    counts = (ctypes.c_uint32 * 8)(4, 0, 0, 0, 0, 0, 0, 0)
    assert lib.cnerf_mesh_atlas_sized_tspace(one, None, 8, one, 4, 48, counts, one, BIG, one, 0, 16, one, 3, one, one, 16, None) == -1   # R no power of two
    assert lib.cnerf_mesh_atlas_sized_tspace(one, None, 8, one, 4, 64, counts, None, BIG, one, 0, 16, one, 3, one, one, 16, None) == -2
    assert lib.cnerf_mesh_atlas_sized_tspace(one, None, 8, one, 4, 64, counts, one, BIG, one, 0, 33, one, 3, one, one, 16, None) == -1   # past the 2 cells
    assert lib.cnerf_mesh_atlas_sized_tspace(one, None, 8, one, 4, 64, counts, one, BIG, None, 0, 16, one, 3, one, one, 16, None) == -2
    assert lib.cnerf_mesh_atlas_proj_tspace(one, None, 8, one, 4, 8, one, BIG, one, 0, 16, one, 3, one, one, 16, None) == -1
    assert lib.cnerf_mesh_atlas_proj_tspace(one, None, 8, one, 4, 64, None, BIG, one, 0, 16, one, 3, one, one, 16, None) == -2
    assert lib.cnerf_mesh_atlas_proj_tspace(one, None, 8, one, 4, 64, one, 16, one, 0, 16, one, 3, one, one, 16, None) == -1
    assert lib.cnerf_mesh_atlas_proj_tspace(one, None, 8, one, 4, 64, one, BIG, one, 0, 64 * 64 + 1, one, 3, one, one, 16, None) == -1
    assert lib.cnerf_mesh_atlas_proj_tspace(one, None, 8, one, 4, 64, one, BIG, None, 0, 16, one, 3, one, one, 16, None) == -2
