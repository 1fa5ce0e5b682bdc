"""CPU: the ray rule of csrc/mesh_bvh.hip as tests/ray_restatement.py restates it — against facts that need no GPU: analytic hits,
watertightness on a closed icosphere (with the float64 branch taken), the cull modes, ties, degenerate rays, the ambient-occlusion
directions and frame — and the argument checks of the C entry points that return before any launch."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ray_restatement as RR  # noqa: E402
import ray_testlib as T  # noqa: E402

F32 = np.float32
TRI_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
TRI_F = np.array([[0, 1, 2]], np.int32)


def test_analytic_hits():
    """rays down the axis of the unit triangle: t is the height, the barycentrics are (1 - x - y, x, y); unnormalised directions scale t"""
    pts = np.array([[0.25, 0.25], [0.125, 0.5], [0.5, 0.125], [0.0625, 0.0625]], F32)
    for h, scale in ((2.0, 1.0), (0.5, 4.0), (3.0, 0.25)):
        o = np.concatenate([pts, np.full((len(pts), 1), h, F32)], 1)
        d = np.tile(np.array([[0, 0, -scale]], F32), (len(pts), 1))
        r = RR.cast(TRI_V, TRI_F, o, d)['none']
        assert (r['face'] == 0).all() and r['occluded'].all()
        np.testing.assert_array_equal(r['t'], np.full(len(pts), h / scale, F32))
        np.testing.assert_array_equal(r['bary'], np.stack([1 - pts[:, 0] - pts[:, 1], pts[:, 0], pts[:, 1]], 1))
    # beside the triangle, behind the origin, beyond t_max, before t_min
    o = np.array([[0.75, 0.75, 1], [0.25, 0.25, -1], [0.25, 0.25, 1], [0.25, 0.25, 1]], F32)
    d = np.tile(np.array([[0, 0, -1]], F32), (4, 1))
    r = RR.cast(TRI_V, TRI_F, o, d, np.array([0, 0, 0, 1.5], F32), np.array([np.inf, np.inf, 0.5, 9], F32))['none']
    assert (r['face'] == -1).all() and np.isposinf(r['t']).all() and not r['occluded'].any() and (r['bary'] == 0).all()
    # an oblique ray: the hit point from t and from the barycentrics agree
    o, d = np.array([[2.0, -1.0, 3.0]], F32), np.array([[-1.75, 1.3, -3.0]], F32)
    r = RR.cast(TRI_V, TRI_F, o, d)['none']
    assert r['face'][0] == 0 and abs(r['t'][0] - 1.0) < 1e-6
    np.testing.assert_allclose(r['bary'][0] @ TRI_V, (o + r['t'][0] * d)[0], atol=1e-6)


def test_watertight_icosphere():
    """every vertex, edge midpoint and face centroid of a closed icosphere, as float32 targets from interior origins, is hit at the target;
    the float64 branch is taken in this set (from the centre every shared edge and vertex is met exactly or nearly so)"""
    v, f = T.icosphere(2)
    tg = T.targets(v, f)
    assert len(tg) == 162 + 480 + 320
    taken = 0
    for origin in (np.zeros(3, F32), np.array([0.013, -0.021, 0.017], F32), np.array([0.5, 0.25, -0.125], F32)):
        o, d = T.rays_to(origin, tg)
        r = RR.cast(v, f, o, d)
        taken += r['fallbacks']
        r = r['none']
        assert r['occluded'].all() and (r['face'] >= 0).all()
        dist = np.linalg.norm(tg.astype(np.float64) - origin, axis=1)
        hit = np.linalg.norm(r['t'][:, None].astype(np.float64) * d, axis=1)
        assert (np.abs(hit - dist) <= 1e-5 * dist).all()
        # the hit face is one that holds the target: its barycentric point is the target
        p = np.einsum('qk,qkc->qc', r['bary'].astype(np.float64), v[f[r['face']]].astype(np.float64))
        assert np.abs(p - tg).max() < 1e-5
    print(f"{taken} (ray, face) pairs took the float64 branch")
    assert taken >= 1
    # and rays built to zero an edge function: axis-aligned, through vertices with integer coordinates
    ov, of = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32), \
        np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    d = np.concatenate([ov, ov])
    o = np.concatenate([np.zeros((6, 3), F32), -3 * ov])
    r = RR.cast(ov, of, o, d)
    assert r['fallbacks'] >= 12 and r['none']['occluded'].all()
    np.testing.assert_array_equal(r['none']['t'], np.concatenate([np.ones(6, F32), np.full(6, 2, F32)]))   # from outside: the near vertex


def test_cull_modes():
    """one face wound counter-clockwise seen from +z: from above its front is met, from below its back"""
    o = np.array([[0.25, 0.25, 1], [0.25, 0.25, -1]], F32)
    d = np.array([[0, 0, -1], [0, 0, 1]], F32)
    r = RR.cast(TRI_V, TRI_F, o, d, culls=('none', 'back', 'front'))
    assert r['none']['face'].tolist() == [0, 0] and r['back']['face'].tolist() == [0, -1] and r['front']['face'].tolist() == [-1, 0]
    assert r['back']['occluded'].tolist() == [True, False] and r['front']['occluded'].tolist() == [False, True]
    # a closed mesh wound outwards: from outside 'back' keeps the near side, 'front' the far side
    v, f = T.icosphere(1)
    o, d = np.array([[0.1, 0.2, 3.0]], F32), np.array([[0, 0, -1]], F32)
    r = RR.cast(v, f, o, d, culls=('none', 'back', 'front'))
    assert r['none']['t'][0] == r['back']['t'][0] < 3.0 < r['front']['t'][0]


def test_ties_take_the_smaller_index():
    v = np.concatenate([TRI_V, TRI_V, TRI_V + np.array([0, 0, 1], F32)])
    f = np.array([[6, 7, 8], [3, 4, 5], [0, 1, 2], [2, 0, 1]], np.int32)         # faces 1, 2 and 3 coincide; face 0 lies behind them
    o, d = np.array([[0.25, 0.25, -1]], F32), np.array([[0, 0, 1]], F32)
    r = RR.cast(v, f, o, d)['none']
    assert r['face'][0] == 1 and r['t'][0] == 1.0
    r = RR.cast(v, f[::-1].copy(), o, d)['none']
    assert r['face'][0] == 0 and r['t'][0] == 1.0


def test_degenerate_rays_miss():
    o = np.array([r[0] for r in T.DEGENERATE], F32) + np.array([0.25, 0.25, 0], F32)
    d = np.array([r[1] for r in T.DEGENERATE], F32)
    big = np.array([[-9, -9, 0], [9, -9, 0], [0, 9, 0], [-9, -9, -1], [9, -9, -1], [0, 9, -1]], F32)       # hard to miss otherwise
    r = RR.cast(big, np.array([[0, 1, 2], [3, 4, 5]], np.int32), o, d, np.array([x[2] for x in T.DEGENERATE], F32),
                np.array([x[3] for x in T.DEGENERATE], F32), culls=('none', 'back', 'front'))
    for k in ('none', 'back', 'front'):
        assert (r[k]['face'] == -1).all() and np.isposinf(r[k]['t']).all() and not r[k]['occluded'].any()
    # the same geometry does stop a proper ray; faces left out of the tree take no part
    assert RR.cast(big, np.array([[0, 1, 2]], np.int32), [[0.25, 0.25, -5]], [[0, 0, 1]])['none']['face'][0] == 0
    bad = big.copy()
    bad[1, 1] = np.nan
    r = RR.cast(bad, np.array([[0, 1, 2], [3, 4, 9], [3, 4, 5]], np.int32), [[0.25, 0.25, 5]], [[0, 0, -1]])['none']
    assert r['face'][0] == 2 and r['t'][0] == 6.0


def test_ao_directions_and_frame():
    for K in (1, 2, 16, 64, 1000):
        d = RR.ao_directions(K).astype(np.float64)
        assert d.shape == (K, 3) and (np.abs(np.linalg.norm(d, axis=1) - 1) <= 1e-6).all() and (d[:, 2] > 0).all()
        assert abs(d[:, 2].mean() - 2.0 / 3.0) <= 1.0 / K                          # the cosine-weighted expectation of z
    d = RR.ao_directions(4096).astype(np.float64)
    assert abs(d[:, 0].mean()) < 5e-3 and abs(d[:, 1].mean()) < 5e-3 and abs((d[:, 0] ** 2).mean() - 0.25) < 5e-3
    rng = np.random.default_rng(0)
    n = rng.standard_normal((200, 3))
    n = np.concatenate([n / np.linalg.norm(n, axis=1, keepdims=True), [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0]]]).astype(F32)
    b1, b2 = (x.astype(np.float64) for x in RR.basis(n))
    n64 = n.astype(np.float64)
    for a, b, want in ((b1, b1, 1), (b2, b2, 1), (b1, b2, 0), (b1, n64, 0), (b2, n64, 0)):
        assert np.abs((a * b).sum(1) - want).max() < 1e-6
    assert np.abs(np.cross(b1, b2) - n64).max() < 1e-6                             # right-handed: b1 x b2 = n
    org, dirs = RR.ao_rays(np.zeros_like(n), 3 * n, 16, 0.5)                       # the normals need not be unit
    assert np.abs(org - 0.5 * n[:, None]).max() < 1e-6 and np.abs(np.linalg.norm(dirs, axis=2) - 1).max() < 1e-5
    assert ((dirs * n[:, None]).sum(2) > 0).all()                                  # every ray leaves on the normal's side


def test_brute_force_ambient_occlusion():
    """a floor under a ceiling half as large: the vertex under the ceiling's middle is darker than the one under its corner; an unused
    vertex is open"""
    floor = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.25, 0.25, 0], [9, 9, 9]], F32)
    ceil = np.array([[0, 0, 0.2], [0.5, 0, 0.2], [0, 0.5, 0.2], [0.5, 0.5, 0.2]], F32)
    v = np.concatenate([floor, ceil])
    f = np.array([[0, 1, 4], [1, 3, 4], [3, 2, 4], [2, 0, 4], [6, 7, 8], [7, 9, 8]], np.int32)
    n = np.tile(np.array([[0, 0, 1]], F32), (len(v), 1))
    org, d = RR.ao_rays(v, n, 64, 1e-4)
    ao, free = RR.ambient_occlusion(v, f, org, d)
    assert ao[5] == 1.0 and ao[4] < ao[0] < 1.0 and ao[4] < 0.6 and (ao[6:] == 1.0).all()
    assert RR.ambient_occlusion(v, f, org, d, radius=0.1)[0].min() == 1.0          # the ceiling is farther than the radius


def test_abi_argument_checks():
    """the ray entry points: NULL and out-of-range arguments return before any launch (no GPU work is issued here)"""
    from customnerf_amd import _lib
    lib = _lib.lib
    need = C.c_uint64(0)
    assert lib.cnerf_mesh_bvh_workspace_bytes(1000, 2000, C.byref(need)) == 0
    one, odd, big = C.c_void_p(4096), C.c_void_p(4097), 1 << 40
    inf = float("inf")
    rc = lib.cnerf_mesh_bvh_raycast
    assert rc(None, big, 1000, 2000, one, one, 8, 0.0, inf, None, None, 0, one, one, None, None, None) == -2
    assert rc(one, big, 1000, 2000, None, one, 8, 0.0, inf, None, None, 0, one, one, None, None, None) == -2
    assert rc(one, big, 1000, 2000, one, None, 8, 0.0, inf, None, None, 0, one, one, None, None, None) == -2
    assert rc(one, need.value - 1, 1000, 2000, one, one, 8, 0.0, inf, None, None, 0, one, one, None, None, None) == -1
    assert rc(odd, big, 1000, 2000, one, one, 8, 0.0, inf, None, None, 0, one, one, None, None, None) == -1
    assert rc(one, big, 1000, 2000, one, one, 1 << 31, 0.0, inf, None, None, 0, one, one, None, None, None) == -1
    assert rc(one, big, 1000, 1 << 31, one, one, 8, 0.0, inf, None, None, 0, one, one, None, None, None) == -1
    for cull in (-1, 3):
        assert rc(one, big, 1000, 2000, one, one, 8, 0.0, inf, None, None, cull, one, one, None, None, None) == -1
    assert rc(one, big, 1000, 2000, None, None, 0, 0.0, inf, None, None, 0, None, None, None, None, None) == 0     # no ray: no launch
    oc = lib.cnerf_mesh_bvh_occluded
    assert oc(None, big, 1000, 2000, one, one, 8, 0.0, inf, None, None, 0, one, None, None) == -2
    assert oc(one, big, 1000, 2000, one, one, 8, 0.0, inf, None, None, 0, None, None, None) == -2
    assert oc(one, big, 1000, 2000, None, one, 8, 0.0, inf, None, None, 0, one, None, None) == -2
    assert oc(one, need.value - 1, 1000, 2000, one, one, 8, 0.0, inf, None, None, 0, one, None, None) == -1
    assert oc(one, big, 1000, 2000, one, one, 1 << 31, 0.0, inf, None, None, 0, one, None, None) == -1
    assert oc(one, big, 1000, 2000, one, one, 8, 0.0, inf, None, None, 3, one, None, None) == -1
    assert oc(one, big, 1000, 2000, None, None, 0, 0.0, inf, None, None, 0, None, None, None) == 0
    from customnerf_amd import mesh
    for name in ("ray_cast", "occluded", "ao_directions", "ao_rays", "ambient_occlusion"):
        assert callable(getattr(mesh, name))
    np.testing.assert_array_equal(mesh.ao_directions(64).numpy().view(np.uint32), RR.ao_directions(64).view(np.uint32))
