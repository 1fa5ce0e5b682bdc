"""CPU: the rules of the mesh rasteriser (include/customnerf_hip.h, cnerf_mesh_raster_*) through their NumPy restatement
(tests/raster_restatement.py) — watertight coverage of a planar grid and of a closed sphere, culling, the analytic sphere's mask and depth —
and the argument checks of the new entry points, which return before any launch.  No GPU compute is issued here."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mc_restatement as R  # noqa: E402
import raster_restatement as RS  # noqa: E402
from mesh_testlib import grid, lattice  # noqa: E402

N_SPHERE, R_SPHERE = 40, 0.9
STEP = 2.0 / (N_SPHERE - 1)


def sphere_mesh(n=N_SPHERE, r=R_SPHERE):
    (X, Y, Z), sp = lattice((n, n, n), -1.0, 1.0)
    return R.marching_cubes((r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))


@pytest.fixture(scope="module")
def sphere_view():
    from customnerf_amd import scene
    v, f, _ = sphere_mesh()
    c2w, intr = scene.camera_pose(3), scene.intrinsics(128, 128)
    return v, f, c2w, intr, RS.visibility(v, f, c2w, intr, 128, 128, count_cover=True)


@pytest.mark.parametrize("convention", ["nerfstudio", "ngp"])
def test_planar_grid_is_covered_once(convention):
    from customnerf_amd import scene
    v, f = grid(16)
    v = v.copy()
    v[:, :2] = v[:, :2] / 8.0 - 1.0                                          # recentred to [-1, 1]^2
    H, W = 96, 128
    c2w = scene.camera_pose(1, elev_deg=35, opencv=convention == "ngp")
    vis = RS.visibility(v, f, c2w, scene.intrinsics(H, W), H, W, convention=convention, count_cover=True)
    assert vis['dropped'] == 0 and not vis['bad']
    assert vis['cover'].max() == 1                                           # shared edges and vertices belong to exactly one face
    assert int((vis['cover'] == 1).sum()) == 2248
    assert np.array_equal(vis['face'] >= 0, vis['cover'] == 1)
    hit = vis['face'] >= 0
    np.testing.assert_allclose(vis['bary'][hit].sum(-1), 1.0, atol=1e-5)
    assert (vis['bary'][hit] >= 0).all() and np.isinf(vis['depth'][~hit]).all() and (vis['bary'][~hit] == 0).all()


def test_closed_sphere_is_covered_twice(sphere_view):
    v, f, c2w, intr, vis = sphere_view
    assert vis['dropped'] == 0 and not vis['bad']
    hit = vis['face'] >= 0
    assert hit.sum() > 1000
    assert (vis['cover'][hit] == 2).all() and (vis['cover'][~hit] == 0).all()      # one front and one back face, no crack, no overlap
    back = RS.visibility(v, f, c2w, intr, 128, 128, cull='back')
    assert np.array_equal(back['face'], vis['face'])
    np.testing.assert_array_equal(back['depth'].view(np.uint32), vis['depth'].view(np.uint32))
    tri = v[f[vis['face'][hit]]].astype(np.float64)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((nrm * (tri[:, 0] - c2w[:, 3].astype(np.float64))).sum(-1) < 0).all()  # every winner faces the camera
    front = RS.visibility(v, f, c2w, intr, 128, 128, cull='front')
    assert np.array_equal(front['face'] >= 0, hit) and (front['depth'][hit] > vis['depth'][hit]).all()


def pixel_rays(c2w, intr, H, W):
    """'nerfstudio' rays through the pixel centres: origin o [3], unit directions d [H, W, 3], |camera-space direction| [H, W] (z = -1)"""
    fx, fy, cx, cy = intr
    iy, ix = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cam = np.stack([(ix + 0.5 - cx) / fx, -(iy + 0.5 - cy) / fy, -np.ones_like(ix, float)], -1)
    ln = np.linalg.norm(cam, axis=-1)
    m = c2w.astype(np.float64)
    return m[:, 3], (cam @ m[:, :3].T) / ln[..., None], ln


def test_restatement_against_analytic_sphere(sphere_view):
    """Outside the band of pixels whose ray passes within one lattice step h of the silhouette (at most 8 % of the image) the mask is the
    analytic sphere's and the depth is within h / 4 of the analytic camera-axis depth (the chord error of the mesh is about h^2 / r)."""
    v, f, c2w, intr, vis = sphere_view
    o, d, ln = pixel_rays(c2w, intr, 128, 128)
    od = (d * o).sum(-1)
    dist = np.linalg.norm(o - od[..., None] * d, axis=-1)
    band = np.abs(dist - R_SPHERE) <= STEP
    share = band.mean()
    print(f"band share {share:.4f}")
    assert share <= 0.08
    hit = vis['face'] >= 0
    want = dist < R_SPHERE
    print(f"mask mismatches outside the band {int((hit != want)[~band].sum())}, over the image {int((hit != want).sum())}")
    assert np.array_equal(hit[~band], want[~band])
    sel = want & ~band
    depth = (-od - np.sqrt(np.maximum(R_SPHERE ** 2 - dist ** 2, 0.0))) / ln
    err = np.abs(vis['depth'][sel] - depth[sel]).max()
    print(f"worst depth error {err:.5f} (bound {STEP / 4:.5f})")
    assert err <= STEP / 4


def test_near_drops_faces_whole():
    from customnerf_amd import scene
    v, f, _ = sphere_mesh(20)
    c2w = scene.camera_pose(0, radius=0.5, elev_deg=10)                      # inside the sphere: part of it lies behind the camera
    intr = scene.intrinsics(48, 64)
    vis = RS.visibility(v, f, c2w, intr, 48, 64, count_cover=True)
    _, _, _, ok, z = RS.project(v, c2w, intr)
    assert 0 < vis['dropped'] == int((~ok[f].all(1)).sum()) < len(f)
    assert (z[f[vis['face'][vis['face'] >= 0]]] >= np.float32(0.01)).all()
    assert vis['cover'].max() == 1 and (vis['face'] >= 0).sum() > 100        # only the far wall is seen, once
    front = RS.visibility(v, f, c2w, intr, 48, 64, cull='front')             # the inside of an outward-wound wall is back-facing
    assert np.array_equal(front['face'], vis['face'])
    assert (RS.visibility(v, f, c2w, intr, 48, 64, cull='back')['face'] == -1).all()


def test_shading_restatement():
    from customnerf_amd import scene
    v, f, n = sphere_mesh(16)
    c2w, intr = scene.camera_pose(2), scene.intrinsics(40, 56)
    vis = RS.visibility(v, f, c2w, intr, 40, 56)
    hit = vis['face'] >= 0
    img, mask = RS.shade(vis, v, f, 'normals', normals=n, bg=(1, 2, 3))
    assert np.array_equal(mask == 255, hit) and (img[~hit] == (1, 2, 3)).all()
    p = (vis['bary'][hit][..., None] * v[f[vis['face'][hit]]]).sum(1)
    want = 0.5 + 0.5 * p / np.linalg.norm(p, axis=1, keepdims=True)          # the sphere's normal is its position
    assert np.abs(img[hit] / 255.0 - want).max() < 0.03
    col = np.clip(np.rint((0.5 + 0.4 * v) * 255), 0, 255).astype(np.uint8)
    img, _ = RS.shade(vis, v, f, 'colors', colors=col)
    assert np.abs(img[hit] / 255.0 - (0.5 + 0.4 * p)).max() <= 1.01 / 255
    d0, d1 = float(vis['depth'][hit].min()), float(vis['depth'][hit].max())
    img, _ = RS.shade(vis, v, f, 'depth', depth_range=(d0, d1))
    assert img[hit].min() == 0 and img[hit].max() == 255 and (img[..., 0] == img[..., 2]).all()
    assert np.array_equal(RS.to_u8(np.array([np.nan, -1.0, 0.5, 2.5 / 255, 3.5 / 255, 2.0], np.float32)), [0, 0, 128, 2, 4, 255])


def test_argument_validation_without_launch():
    """Rejected arguments return before anything touches the device (safe without a GPU); the dummy pointers are never dereferenced."""
    from customnerf_amd._lib import lib
    one = ctypes.c_void_p(16)
    need = ctypes.c_uint64(0)
    assert lib.cnerf_mesh_raster_workspace_bytes(10, 20, 30, 40, ctypes.addressof(need)) == 0
    assert need.value >= 8 * 30 * 40 + 16 * 10 + 20 * 20 and need.value % 256 == 0
    small = need.value
    assert lib.cnerf_mesh_raster_workspace_bytes(0, 0, 0, 0, ctypes.addressof(need)) == 0 and need.value % 256 == 0
    assert lib.cnerf_mesh_raster_workspace_bytes(10, 20, 30, 40, None) == -2
    assert lib.cnerf_mesh_raster_workspace_bytes(1 << 31, 20, 30, 40, ctypes.addressof(need)) == -1
    assert lib.cnerf_mesh_raster_workspace_bytes(10, 20, 1 << 16, 1 << 15, ctypes.addressof(need)) == -1        # H W = 2^31
    c2w = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 3)

    def vis(**over):
        a = dict(verts=one, V=10, faces=one, F=20, c2w=c2w, fx=50.0, fy=50.0, cx=20.0, cy=15.0, H=30, W=40, convention=0, near=0.01, cull=0,
                 ws=one, ws_bytes=1 << 40, face=one, depth=one, bary=one, counts=one)
        a.update(over)
        return lib.cnerf_mesh_raster_visibility(a["verts"], a["V"], a["faces"], a["F"], a["c2w"], a["fx"], a["fy"], a["cx"], a["cy"], a["H"],
                                                a["W"], a["convention"], a["near"], a["cull"], a["ws"], a["ws_bytes"], a["face"], a["depth"],
                                                a["bary"], a["counts"], None)
    for bad in (dict(fx=0.0), dict(fy=0.0), dict(fx=float("nan")), dict(fy=float("inf")), dict(near=float("nan")), dict(near=float("inf")),
                dict(H=1 << 16, W=1 << 15), dict(V=1 << 31), dict(convention=2), dict(convention=-1), dict(cull=3), dict(cull=-1),
                dict(ws_bytes=small - 1), dict(ws=ctypes.c_void_p(24))):
        assert vis(**bad) == -1, bad
    for null in ("verts", "faces", "c2w", "ws", "face", "depth", "bary", "counts"):
        assert vis(**{null: None}) == -2, null
    bg = (ctypes.c_uint8 * 3)(0, 0, 0)

    def shade(**over):
        a = dict(face=one, depth=one, bary=one, H=30, W=40, faces=one, V=10, F=20, mode=0, colors=one, uvs=one, texture=one, R=64, verts=one,
                 normals=one, d0=0.0, d1=1.0, bg=bg, image=one, mask=one)
        a.update(over)
        return lib.cnerf_mesh_raster_shade(a["face"], a["depth"], a["bary"], a["H"], a["W"], a["faces"], a["V"], a["F"], a["mode"], a["colors"],
                                           a["uvs"], a["texture"], a["R"], a["verts"], a["normals"], a["d0"], a["d1"], a["bg"], a["image"],
                                           a["mask"], None)
    for bad in (dict(mode=4), dict(mode=-1), dict(mode=1, R=0), dict(mode=1, R=16385), dict(H=1 << 16, W=1 << 15), dict(V=1 << 31)):
        assert shade(**bad) == -1, bad
    for null in (dict(bg=None), dict(face=None), dict(bary=None), dict(image=None), dict(mask=None), dict(faces=None), dict(colors=None),
                 dict(mode=1, uvs=None), dict(mode=1, texture=None), dict(mode=2, normals=None), dict(mode=2, verts=None),
                 dict(mode=3, depth=None)):
        assert shade(**null) == -2, null
    assert shade(H=0) == 0                                                      # no pixel: accepted without a launch


def test_abi_version_and_python_surface():
    from customnerf_amd import _lib, mesh
    from customnerf_amd.nerf.renderer import NeRFRenderer
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8
    assert mesh.raster_workspace_bytes(10, 20, 30, 40) >= 8 * 30 * 40 + 16 * 10 + 20 * 20
    assert callable(mesh.rasterize) and callable(mesh.render_mesh) and callable(NeRFRenderer.render_mesh)
    with pytest.raises(ValueError):
        mesh.raster_workspace_bytes(10, 20, 1 << 16, 1 << 15)
