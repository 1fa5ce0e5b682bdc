"""CPU: the texture atlas of csrc/mesh_texture.hip through its NumPy restatement (tests/atlas_restatement.py) — layout numbers against the
library's host-side layout, the seam invariant checked exhaustively, UV winding — and the PNG / OBJ / MTL writers of customnerf_amd/mesh.py.
No GPU compute is issued here."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import atlas_restatement as A  # noqa: E402

# (F, R): odd and even F, one face, a lone odd face in the last cell, R not a multiple of n, cells of exactly 4 texels, a large count
SEAM_CASES = [(1, 16), (2, 16), (3, 16), (7, 40), (9, 37), (31, 16), (32, 16), (50, 64), (101, 100), (257, 203), (1999, 256)]


def test_layout_numbers():
    from customnerf_amd import mesh
    table = {(0, 16): (1, 16), (1, 16): (1, 16), (2, 16): (1, 16), (3, 16): (2, 8), (31, 16): (4, 4), (32, 16): (4, 4),
             (9, 37): (3, 12), (1000, 256): (23, 11), (100_000, 2048): (224, 9), (2, 16384): (1, 16384)}
    for (F, R), ns in table.items():
        assert mesh.atlas_layout(F, R) == ns, (F, R)
        assert A.layout(F, R) == ns, (F, R)
    rng = np.random.default_rng(3)
    for F, R in zip(rng.integers(0, 2_000_000, 300), rng.integers(16, 16385, 300)):
        F, R = int(F), int(R)
        try:
            ref = A.layout(F, R)
        except ValueError:
            with pytest.raises(ValueError, match="decimate"):
                mesh.atlas_layout(F, R)
            continue
        assert mesh.atlas_layout(F, R) == ref, (F, R)
        n, s = ref
        P = (F + 1) // 2
        assert (n - 1) ** 2 < max(P, 1) <= n * n and s == R // n >= 4 and P <= n * n


def test_layout_errors():
    from customnerf_amd import mesh
    with pytest.raises(ValueError, match="decimate the mesh"):
        mesh.atlas_layout(33, 16)                                    # P = 17 -> n = 5, s = 3
    assert mesh.atlas_layout(100_000, 1024) == (224, 4)
    with pytest.raises(ValueError, match="decimate the mesh"):
        mesh.atlas_layout(100_000, 895)                            # 895 // 224 = 3
    for F, R in ((10, 15), (10, 16385), (-1, 64), (2 ** 31, 64)):
        with pytest.raises(ValueError):
            mesh.atlas_layout(F, R)


def _triangle_samples(c, rng, k_edge=9, k_in=40):
    """points of the triangle with corners c [3, 2] (texel coordinates): corners, points along every edge, random interior points"""
    pts = [c]
    t = np.arange(1, k_edge)[:, None] / k_edge
    for a, b in ((0, 1), (1, 2), (2, 0)):
        pts.append(c[a] + t * (c[b] - c[a]))
    w = rng.random((k_in, 3)) + 1e-3
    w /= w.sum(1, keepdims=True)
    pts.append(w @ c)
    return np.concatenate(pts)


@pytest.mark.parametrize("F,R", SEAM_CASES, ids=[f"F{f}_R{r}" for f, r in SEAM_CASES])
def test_seam_invariant(F, R):
    """Every texel with a nonzero bilinear weight at any point of a face's UV triangle is owned by that face."""
    rng = np.random.default_rng(F * 1000 + R)
    own = A.owner_map(F, R)
    XY = A.corner_texels(F, R).astype(np.float64)                    # texel centres at integer coordinates
    for f in range(F):
        p = _triangle_samples(XY[f], rng)
        x0, y0 = np.floor(p[:, 0]).astype(np.int64), np.floor(p[:, 1]).astype(np.int64)
        fx, fy = p[:, 0] > x0, p[:, 1] > y0
        for dx, dy, m in ((0, 0, np.ones(len(p), bool)), (1, 0, fx), (0, 1, fy), (1, 1, fx & fy)):
            X, Y = x0[m] + dx, y0[m] + dy
            assert ((X >= 0) & (X < R) & (Y >= 0) & (Y < R)).all(), (F, R, f)
            assert (own[Y, X] == f).all(), (F, R, f)
    # owned texels: P cells of s^2, less the B half of the last cell when F is odd
    n, s = A.layout(F, R)
    assert (own >= 0).sum() == (F + 1) // 2 * s * s - (F % 2) * (s * s - s * (s + 1) // 2)


@pytest.mark.parametrize("F,R", SEAM_CASES, ids=[f"F{f}_R{r}" for f, r in SEAM_CASES])
def test_uvs_decode_to_corner_texels_and_wind_ccw(F, R):
    uv = A.uvs(F, R).astype(np.float64)
    XY = A.corner_texels(F, R)
    px, py = uv[..., 0] * R - 0.5, (1 - uv[..., 1]) * R - 0.5
    assert np.abs(px - XY[..., 0]).max() < 1e-3 and np.abs(py - XY[..., 1]).max() < 1e-3
    e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0).all()     # counter-clockwise with v up


def test_points_restatement_affine_and_corners():
    """x at the corner texels is the vertex; x is affine in (i, j) over a face's texels; d is the unit inward normal of a flat face"""
    rng = np.random.default_rng(5)
    F, R = 9, 64
    V = rng.standard_normal((F * 3, 3)).astype(np.float32)
    fc = np.arange(F * 3, dtype=np.int32).reshape(F, 3)
    n, s = A.layout(F, R)
    x, d = A.points(V, fc, R)
    face, i, j, X, Y = A.cell_texels(F, R)
    XY = A.corner_texels(F, R)
    for f in range(F):
        for k in range(3):
            t = np.nonzero((X == XY[f, k, 0]) & (Y == XY[f, k, 1]))[0][0]
            assert face[t] == f and np.array_equal(x[t], V[fc[f, k]])
        m = face == f
        g = np.cross(V[fc[f, 1]] - V[fc[f, 0]], V[fc[f, 2]] - V[fc[f, 0]]).astype(np.float64)
        np.testing.assert_allclose(d[m], np.tile(-g / np.linalg.norm(g), (m.sum(), 1)), atol=1e-6)
        A_ = np.stack([np.ones(m.sum()), i[m], j[m]], 1).astype(np.float64)
        coef, *_ = np.linalg.lstsq(A_, x[m].astype(np.float64), rcond=None)
        np.testing.assert_allclose(A_ @ coef, x[m], atol=1e-5)
    assert (face[(F + 1) // 2 * s * s - 1:] == -1).all() and (x[face < 0] == 0).all() and (d[face < 0] == [0, 0, -1]).all()


def test_png_round_trip(tmp_path):
    from customnerf_amd import mesh
    img = np.random.default_rng(1).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    p = str(tmp_path / "t.png")
    mesh.write_png(p, img)
    np.testing.assert_array_equal(A.read_png(p), img)
    Image = pytest.importorskip("PIL.Image")
    with Image.open(p) as im:
        assert im.mode == "RGB" and im.size == (53, 37)
        np.testing.assert_array_equal(np.asarray(im), img)
    with pytest.raises(ValueError):
        mesh.write_png(p, img[..., :2])


def test_obj_structure(tmp_path):
    from customnerf_amd import mesh
    rng = np.random.default_rng(2)
    v = rng.standard_normal((10, 3)).astype(np.float32) * np.float32(1e3)
    f = rng.integers(0, 10, (7, 3)).astype(np.int32)
    nrm = rng.standard_normal((10, 3)).astype(np.float32)
    R = 32
    uv = A.uvs(len(f), R)
    tex = rng.integers(0, 256, (R, R, 3), dtype=np.uint8)
    p = str(tmp_path / "mesh.obj")
    mesh.write_obj(p, v, f, uvs=uv, normals=nrm, texture=tex)
    o = A.read_obj(p)
    assert np.array_equal(o["verts"], v) and np.array_equal(o["normals"], nrm) and np.array_equal(o["uvs"], uv.reshape(-1, 2))
    assert o["f"].shape == (7, 3, 3)
    assert np.array_equal(o["f"][..., 0], f + 1) and np.array_equal(o["f"][..., 2], f + 1)                  # 1-based
    assert np.array_equal(o["f"][..., 1], np.arange(1, 22).reshape(7, 3))
    assert o["mtllib"] == "mesh.mtl"
    mtl = open(str(tmp_path / "mesh.mtl")).read().split("\n")
    assert "newmtl material0" in mtl and "map_Kd mesh.png" in mtl
    assert "usemtl material0" in open(p).read().split("\n")
    np.testing.assert_array_equal(A.read_png(str(tmp_path / "mesh.png")), tex)
    # plain forms: positions only, positions + normals, positions + uvs
    for kw, k in (({}, 1), ({"normals": nrm}, 3), ({"uvs": uv}, 2)):
        q = str(tmp_path / "plain.obj")
        mesh.write_obj(q, v, f, **kw)
        o = A.read_obj(q)
        assert o["mtllib"] is None and o["f"].shape == (7, 3, k) and np.array_equal(o["f"][..., 0], f + 1)
        if k == 3:
            assert (o["f"][..., 1] == 0).all() and np.array_equal(o["f"][..., 2], f + 1)                      # f v//vn
    assert not os.path.exists(str(tmp_path / "plain.mtl"))
    mesh.write_obj(str(tmp_path / "empty.obj"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    o = A.read_obj(str(tmp_path / "empty.obj"))
    assert len(o["verts"]) == 0 and len(o["f"]) == 0


def test_argument_errors(tmp_path):
    from customnerf_amd import mesh
    from customnerf_amd.nerf.renderer import NeRFRenderer
    v = np.zeros((3, 3), np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    p = str(tmp_path / "m.obj")
    with pytest.raises(ValueError, match="uvs"):
        mesh.write_obj(p, v, f, uvs=np.zeros((2, 3, 2), np.float32))
    with pytest.raises(ValueError, match="needs uvs"):
        mesh.write_obj(p, v, f, texture=np.zeros((16, 16, 3), np.uint8))
    with pytest.raises(ValueError, match="normals"):
        mesh.write_obj(p, v, f, normals=np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="outside"):
        mesh.write_obj(p, v, np.array([[0, 1, 3]], np.int32))
    with pytest.raises(RuntimeError):                                          # no CPU path
        import torch
        mesh.bake_texture(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]), 16, lambda x, d: x)

    class Stub:
        def extract_mesh(self, **kw):
            raise AssertionError("not reached")
    for path in ("m.ply", "m.PLY", "m"):
        with pytest.raises(ValueError, match=r"\.obj"):
            NeRFRenderer.save_mesh(Stub(), str(tmp_path / path), texture=64)
