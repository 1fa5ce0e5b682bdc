"""CPU: the closest-point and sampler rules of csrc/mesh_bvh.hip as tests/bvh_restatement.py restates them — against an independent float64
point-triangle distance, against analytic bounds read off the mesh itself, the sampler's counting and containment properties, an exact
metamorphic case — and the argument checks of the new entry points, none of which launches anything."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bvh_restatement as B  # noqa: E402
import mc_restatement as R  # noqa: E402
from mesh_testlib import decimate_meshes, grid, lattice  # noqa: E402


def sphere_mesh(n=24, r=0.7):
    (X, Y, Z), sp = lattice((n, n, n), -1.0, 1.0)
    v, f, _ = R.marching_cubes((r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))
    return v, f


def segment_d2(p, a, b):
    ab = b - a
    l2 = (ab * ab).sum(-1)
    t = np.clip(((p - a) * ab).sum(-1) / np.where(l2 > 0, l2, 1.0), 0.0, 1.0)
    r = p - (a + t[:, None] * ab)
    return (r * r).sum(-1)


def independent_d2(p, a, b, c):
    """float64 squared distance from p to each triangle by another route: the foot of the perpendicular when it falls inside the triangle,
    else the nearest of the three edges"""
    p, a, b, c = (np.asarray(t, np.float64) for t in (p, a, b, c))
    n = np.cross(b - a, c - a)
    n2 = (n * n).sum(-1)
    edges = np.minimum(np.minimum(segment_d2(p, a, b), segment_d2(p, b, c)), segment_d2(p, c, a))
    safe = np.where(n2 > 0, n2, 1.0)
    h = ((p - a) * n).sum(-1)
    foot = p - (h / safe)[:, None] * n
    inside = np.ones(len(a), bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(v - u, foot - u) * n).sum(-1) >= 0
    return np.where(inside & (n2 > 0), h * h / safe, edges)


def test_rule_against_independent_float64():
    """the float32 rule, its float64 twin and an independent float64 distance agree: d2 within 1e-5 relative in float64, the float32 one
    within 1e-5 relative plus float32 rounding of coordinates of size 1 against distances of size d"""
    rng = np.random.default_rng(3)
    for name, v, f, _ in decimate_meshes()[:3]:
        a, b, c = (v[f[:, k]] for k in range(3))
        lo, hi = v.min(0), v.max(0)
        for p in rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (12, 3)).astype(np.float32):
            want = independent_d2(p, a, b, c)
            d64, x64, bary64 = B.point_triangles(p, a, b, c, np.float64)
            np.testing.assert_allclose(d64, want, rtol=1e-5, atol=1e-18)
            d32, x32, bary32 = B.point_triangles(p, a, b, c)
            assert d32.dtype == np.float32
            scale = np.abs(v).max() + np.abs(p).max()
            np.testing.assert_allclose(np.sqrt(d32.astype(np.float64)), np.sqrt(want), rtol=1e-5, atol=16 * 6e-8 * scale)
            # the barycentrics describe the closest point and sum to 1
            np.testing.assert_allclose(bary64.sum(1), 1.0, atol=1e-12)
            np.testing.assert_allclose((bary64[:, :, None] * np.stack([a, b, c], 1)).sum(1), x64, atol=1e-12)
            assert (bary32 >= 0).all() and (bary32 <= 1).all()


def test_brute_force_ties_nan_and_left_out_faces():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [np.nan, 0, 0]], np.float32)
    f = np.array([[1, 3, 2], [0, 1, 2], [0, 1, 9], [0, 4, 1], [0, 1, 2]], np.int32)
    ok, flags = B.participating(v, f)
    assert ok.tolist() == [True, True, False, False, True] and flags == 3
    r = B.closest(v, f, [[0.5, 0.5, 1.0], [0.25, 0.25, -2.0], [np.inf, 0, 0], [2.0, 2.0, 0.0]])
    assert r['face'].tolist() == [0, 1, -1, 0]                                  # the shared edge: the smaller index; faces 1 and 4: face 1
    assert r['dist2'].tolist() == [1.0, 4.0, np.inf, 2.0]
    np.testing.assert_array_equal(r['point'][1], [0.25, 0.25, 0.0])
    np.testing.assert_array_equal(r['bary'][3], [0.0, 1.0, 0.0])
    # a face with a == b can give NaN (region 3): it never wins
    v2 = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5]], np.float32)
    f2 = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    r = B.closest(v2, f2, [[0.5, 1.0, 0.0]])
    d2, _, _ = B.point_triangles(np.array([0.5, 1.0, 0.0], np.float32), v2[f2[:, 0]], v2[f2[:, 1]], v2[f2[:, 2]])
    assert np.isnan(d2[0]) and r['face'][0] == 1
    assert B.closest(v, f[:0], [[0, 0, 0]])['face'][0] == -1


def test_analytic_bounds_on_a_sphere():
    """for p outside a marching-cubes sphere mesh: |p| - max|v| <= d <= min_v |p - v| (the mesh lies inside the ball of its farthest
    vertex, and its vertices are points of it)"""
    v, f = sphere_mesh()
    rng = np.random.default_rng(11)
    d = rng.standard_normal((40, 3))
    p = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.8, 3.0, (40, 1))).astype(np.float32)
    got = np.sqrt(B.closest(v, f, p)['dist2'].astype(np.float64))
    lower = np.linalg.norm(p.astype(np.float64), axis=1) - np.linalg.norm(v.astype(np.float64), axis=1).max()
    upper = np.sqrt(((p[:, None, :].astype(np.float64) - v[None].astype(np.float64)) ** 2).sum(-1)).min(1)
    assert (lower > 0).all()
    assert (got >= lower * (1 - 1e-6)).all() and (got <= upper * (1 + 1e-6)).all()
    # and the closest point lies in the reported face: barycentrics in [0, 1] that rebuild it
    r = B.closest(v, f, p)
    tri = v[f[r['face']]].astype(np.float64)
    np.testing.assert_allclose((r['bary'][:, :, None] * tri).sum(1), r['point'], atol=1e-6)


@pytest.mark.parametrize("spacing", [0.31, 0.05, 0.011])
def test_sampler_properties(spacing):
    for name, v, f, _ in decimate_meshes()[:2] + decimate_meshes()[4:]:
        ok, area, k, flags = B.face_orders(v, f, spacing)
        s = B.sample(v, f, spacing)
        assert flags == 0 and ok.all() and s['total'] == int((k * k).sum()) == len(s['points'])
        assert (k >= 1).all() and (np.sqrt(2 * area.astype(np.float64)) / k <= spacing * (1 + 1e-6)).all()
        assert (np.diff(s['face']) >= 0).all() and (np.bincount(s['face'], minlength=len(f)) == k * k).all()
        # the weights of a face sum to its float32 area within the one rounding of A / k^2 (the k^2 equal weights are added in float64); the
        # float32 area of a sliver carries the cancellation of its cross product, so against float64 only the mesh's total is compared
        a64 = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]].astype(np.float64) - v[f[:, 0]], v[f[:, 2]].astype(np.float64) - v[f[:, 0]]), axis=1)
        per_face = np.bincount(s['face'], weights=s['weight'].astype(np.float64), minlength=len(f))
        np.testing.assert_allclose(per_face, area.astype(np.float64), rtol=2 ** -23, atol=0)
        np.testing.assert_allclose(per_face.sum(), a64.sum(), rtol=1e-5)
        # every sample lies in its face, strictly inside, and is where its barycentrics say; no two samples of a face coincide
        b = s['bary'].astype(np.float64)
        assert (b > 0).all() and (b < 1).all()
        np.testing.assert_allclose(b.sum(1), 1.0, atol=2e-7)
        tri = v[f[s['face']]].astype(np.float64)
        np.testing.assert_allclose((b[:, :, None] * tri).sum(1), s['points'], atol=4e-7 * np.abs(v).max())
        key = np.round(b * 3 * k[s['face']][:, None]).astype(np.int64)
        assert len(np.unique(np.concatenate([s['face'][:, None], key], 1), axis=0)) == s['total']


def test_sampler_special_faces():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [1000, 0, 0], [0, 1000, 0], [np.inf, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [3, 3, 3], [0, 1, 7], [0, 4, 5], [0, 1, 6]], np.int32)
    s = B.sample(v, f, 0.5)
    ok, area, k, flags = B.face_orders(v, f, 0.5)
    assert ok.tolist() == [True, True, False, True, False] and k.tolist() == [2, 1, 0, 256, 0] and flags == 1 | 2 | 4
    assert s['total'] == 4 + 1 + 256 * 256
    assert s['weight'][4] == 0 and np.array_equal(s['points'][4], [2, 2, 2])       # the zero-area face: one sample of weight 0
    # the enumeration of k = 2: (i, j, up) = (0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)
    want = np.array([[1, 1], [2, 2], [1, 4], [4, 1]], np.float32) / np.float32(6)
    np.testing.assert_array_equal(s['bary'][:4, 1:], want)


def test_shifted_grid_is_exact():
    """a planar grid against itself moved by 0.25 along z: every sample and every vertex is at distance 0.25 exactly, so max = mean = rms =
    hausdorff = 0.25 without any rounding, both ways"""
    v, f = grid(16)
    v2 = v + np.array([0, 0, 0.25], np.float32)
    d = B.distance(v, f, v2, f, 0.4)
    for way in ('a_to_b', 'b_to_a'):
        assert d[way]['max'] == d[way]['mean'] == d[way]['rms'] == 0.25 and d[way]['n_samples'] > 2 * len(f)
    assert d['hausdorff'] == 0.25
    # moved within its plane instead: zero inside, the overhang at the border
    v3 = v + np.array([0.5, 0, 0], np.float32)
    d = B.distance(v, f, v3, f, 0.4)
    assert d['a_to_b']['max'] == 0.5 and d['b_to_a']['max'] == 0.5 and 0 < d['a_to_b']['mean'] < 0.02


def test_argument_validation_without_launch():
    from customnerf_amd._lib import lib
    one = C.c_void_p(256)                                                       # aligned, non-NULL, never dereferenced on these paths
    odd = C.c_void_p(264)
    need, need_s = C.c_uint64(0), C.c_uint64(0)
    assert lib.cnerf_mesh_bvh_workspace_bytes(1000, 2000, C.byref(need)) == 0 and need.value >= 2000 * (48 + 16 + 16)
    assert lib.cnerf_mesh_bvh_workspace_bytes(1000, 2000, None) == -2 and lib.cnerf_mesh_bvh_workspace_bytes(1 << 31, 1, C.byref(need_s)) == -1
    assert lib.cnerf_mesh_bvh_workspace_bytes(1, 1 << 31, C.byref(need_s)) == -1
    assert lib.cnerf_mesh_bvh_workspace_bytes(0, 0, C.byref(need_s)) == 0 and 0 < need_s.value < 4096
    big = 1 << 40
    assert lib.cnerf_mesh_bvh_build(one, 1000, one, 2000, None, big, one, None) == -2
    assert lib.cnerf_mesh_bvh_build(one, 1000, one, 2000, one, big, None, None) == -2
    assert lib.cnerf_mesh_bvh_build(None, 1000, one, 2000, one, big, one, None) == -2
    assert lib.cnerf_mesh_bvh_build(one, 1000, None, 2000, one, big, one, None) == -2
    assert lib.cnerf_mesh_bvh_build(one, 1000, one, 2000, one, need.value - 1, one, None) == -1
    assert lib.cnerf_mesh_bvh_build(one, 1000, one, 2000, odd, big, one, None) == -1
    assert lib.cnerf_mesh_bvh_build(one, 1 << 31, one, 2000, one, big, one, None) == -1
    assert lib.cnerf_mesh_bvh_build(one, 1000, one, 1 << 31, one, big, one, None) == -1
    assert lib.cnerf_mesh_bvh_closest(None, big, 1000, 2000, one, 8, one, one, None, None, None, None) == -2
    assert lib.cnerf_mesh_bvh_closest(one, big, 1000, 2000, None, 8, one, one, None, None, None, None) == -2
    assert lib.cnerf_mesh_bvh_closest(one, big, 1000, 2000, one, 8, None, one, None, None, None, None) == -2
    assert lib.cnerf_mesh_bvh_closest(one, big, 1000, 2000, one, 8, one, None, None, None, None, None) == -2
    assert lib.cnerf_mesh_bvh_closest(one, need.value - 1, 1000, 2000, one, 8, one, one, None, None, None, None) == -1
    assert lib.cnerf_mesh_bvh_closest(odd, big, 1000, 2000, one, 8, one, one, None, None, None, None) == -1
    assert lib.cnerf_mesh_bvh_closest(one, big, 1000, 2000, one, 1 << 31, one, one, None, None, None, None) == -1
    assert lib.cnerf_mesh_bvh_closest(one, big, 1000, 2000, None, 0, None, None, None, None, None, None) == 0      # no query: no launch
    assert lib.cnerf_mesh_sample_workspace_bytes(2000, C.byref(need_s)) == 0 and need_s.value >= 256 + 8 * 8
    assert lib.cnerf_mesh_sample_workspace_bytes(2000, None) == -2 and lib.cnerf_mesh_sample_workspace_bytes(1 << 31, C.byref(need_s)) == -1
    for sp in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.cnerf_mesh_sample_count(one, 1000, one, 2000, sp, one, big, one, None) == -1
        assert lib.cnerf_mesh_sample_emit(one, 1000, one, 2000, sp, one, big, one, one, one, one, 100, None) == -1
    assert lib.cnerf_mesh_sample_count(one, 1000, one, 2000, 0.1, None, big, one, None) == -2
    assert lib.cnerf_mesh_sample_count(one, 1000, one, 2000, 0.1, one, big, None, None) == -2
    assert lib.cnerf_mesh_sample_count(one, 1000, None, 2000, 0.1, one, big, one, None) == -2
    assert lib.cnerf_mesh_sample_count(one, 1000, one, 2000, 0.1, one, 255, one, None) == -1
    assert lib.cnerf_mesh_sample_count(one, 1000, one, 2000, 0.1, odd, big, one, None) == -1
    assert lib.cnerf_mesh_sample_count(one, 1000, one, 1 << 31, 0.1, one, big, one, None) == -1
    assert lib.cnerf_mesh_sample_emit(one, 1000, one, 2000, 0.1, one, big, None, one, one, one, 100, None) == -2
    assert lib.cnerf_mesh_sample_emit(one, 1000, one, 2000, 0.1, one, big, one, one, one, None, 100, None) == -2
    assert lib.cnerf_mesh_sample_emit(one, 1000, one, 2000, 0.1, one, 255, one, one, one, one, 100, None) == -1
    assert lib.cnerf_mesh_sample_emit(one, 1000, one, 2000, 0.1, one, big, None, None, None, None, 0, None) == 0   # room for none: no launch
    assert lib.cnerf_mesh_sample_emit(None, 0, None, 0, 0.1, one, big, None, None, None, None, 100, None) == 0     # no face: no launch


def test_abi_and_python_surface():
    from customnerf_amd import _lib, mesh
    from customnerf_amd.nerf.renderer import NeRFRenderer
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8
    for name in ("cnerf_mesh_bvh_workspace_bytes", "cnerf_mesh_bvh_build", "cnerf_mesh_bvh_closest", "cnerf_mesh_sample_workspace_bytes",
                 "cnerf_mesh_sample_count", "cnerf_mesh_sample_emit"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert mesh.bvh_workspace_bytes(1000, 2000) >= 2000 * 80
    sig = inspect.signature(mesh.closest_point).parameters
    assert [sig[k].default for k in ("want_point", "want_bary", "want_stats")] == [False, False, False]
    assert inspect.signature(mesh.sample_surface).parameters["max_samples"].default == 1 << 26
    sig = inspect.signature(mesh.distance).parameters
    assert sig["spacing"].default is None and sig["symmetric"].default is True and sig["include_vertices"].default is True
    sig = inspect.signature(NeRFRenderer.extract_mesh).parameters
    assert sig["deviation"].default is False and sig["deviation_spacing"].default is None
    import torch
    with pytest.raises(RuntimeError):
        mesh.build_bvh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))  # no CPU path
    with pytest.raises(ValueError):
        mesh.closest_point(object(), torch.zeros(1, 3))
