"""GPU: closest-point queries through the BVH, the surface sampler and mesh.distance (csrc/mesh_bvh.hip) against their NumPy restatement
(tests/bvh_restatement.py) — dist2, face, point and bary bit-equal to brute force over hand-made, marching-cubes and decimation meshes and one
realistic size; the sampler bit-equal; two runs identical byte for byte; the tree prunes; distance's figures; and the deviation report end to
end through NeRFRenderer.extract_mesh."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bvh_restatement as B  # noqa: E402
import mc_restatement as R  # noqa: E402
from mesh_testlib import AABB, R_SPHERE, cuda, decimate_meshes, dtype_guard, gaussian_model, grid, lattice  # noqa: E402,F401

SENTINEL = -7.0
PAD = 8


def sphere_mesh(n=40, r=0.9):
    (X, Y, Z), sp = lattice((n, n, n), -1.0, 1.0)
    return R.marching_cubes((r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))[:2]


def torus_mesh():
    (X, Y, Z), sp = lattice((48, 44, 36), -1.0, 1.0)
    q = np.sqrt(X ** 2 + Y ** 2) - 0.6
    return R.marching_cubes((0.25 - np.sqrt(q ** 2 + Z ** 2)).astype(np.float32), 0.0, sp, (-1.0, -1.0, -1.0))[:2]


def parity_meshes():
    rng = np.random.default_rng(9)
    v = rng.standard_normal((30, 3)).astype(np.float32)
    f = rng.permutation(30).reshape(10, 3).astype(np.int32)
    yield "soup", v, np.concatenate([f, [[0, 0, 1], [2, 2, 2], [0, 1, 2]]]).astype(np.int32)       # with zero-area faces
    yield ("sphere",) + sphere_mesh()
    yield ("torus",) + torus_mesh()
    for name, dv, df, _ in decimate_meshes():
        yield name, dv, df
    sv, sf = sphere_mesh(14)
    bad = sf.copy()
    bad[len(sf) // 3, 1] = len(sv)                                                # out of range: left out, the others take part
    bad[len(sf) // 2, 2] = -1
    sv = sv.copy()
    sv[sf[5, 0]] = np.nan                                                         # and every face at a non-finite vertex
    yield "bad_faces", sv, bad
    yield "no_face", sv[:10], sf[:0]
    yield "one_face", np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32), np.array([[0, 1, 2]], np.int32)


MESHES = list(parity_meshes())


def finite_box(v, f):
    ok, _ = B.participating(v, f)
    p = v[f[ok].ravel()] if ok.any() else np.zeros((1, 3), np.float32)
    return p.min(0), p.max(0)


def queries(v, f, per=96, seed=0):
    """surface samples, the same moved by 2 % of the diagonal, the mesh's vertices, far points, points on the planes of boxes (the mesh's box
    and coordinates taken from its vertices), and non-finite rows"""
    rng = np.random.default_rng(seed)
    lo, hi = finite_box(v, f)
    diag = float(np.linalg.norm(hi.astype(np.float64) - lo)) or 1.0
    s = B.sample(v, f, 0.05 * diag)['points'] if len(f) else np.zeros((0, 3), np.float32)
    s = s[rng.permutation(len(s))[:per]]
    near = (s + rng.standard_normal(s.shape) * 0.02 * diag).astype(np.float32)
    fin = v[np.isfinite(v).all(1)]
    own = fin[rng.permutation(len(fin))[:per]]
    far = (0.5 * (lo + hi) + rng.standard_normal((24, 3)) * diag * np.array([[3.0], [30.0], [3000.0]]).repeat(8, 0)).astype(np.float32)
    planes = rng.uniform(lo - 0.1 * diag, hi + 0.1 * diag, (48, 3)).astype(np.float32)
    for i in range(len(planes)):                                                  # one or two coordinates snapped to a box plane / a vertex
        for a in rng.permutation(3)[:1 + i % 2]:
            planes[i, a] = (lo[a], hi[a], fin[rng.integers(len(fin)), a] if len(fin) else 0.0)[i % 3]
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    return np.concatenate([s, near, own, far, planes, bad]).astype(np.float32)


def gpu_build(v, f, fill=0x5a):
    """cnerf_mesh_bvh_build into an over-allocated workspace -> (ws tensor, nbytes, counts array with its padding, V, F)"""
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib, check, ptr, stream
    gv, gf = cuda(np.asarray(v, np.float32)), cuda(np.asarray(f, np.int32))
    V, F = len(v), len(f)
    nbytes = mesh.bvh_workspace_bytes(V, F)
    ws = torch.full((nbytes + 256,), fill, dtype=torch.uint8, device="cuda")
    counts = torch.full((2 + PAD,), 0x55, dtype=torch.int32, device="cuda")
    check(lib.cnerf_mesh_bvh_build(ptr(gv) if V else None, V, ptr(gf) if F else None, F, ptr(ws), nbytes, ptr(counts), stream()), "build")
    torch.cuda.synchronize()
    assert (ws[nbytes:] == fill).all()
    counts = counts.cpu().numpy()
    assert (counts[2:] == 0x55).all()
    return ws, nbytes, counts, V, F


def gpu_closest(tree, pts, want=("point", "bary", "stats")):
    """cnerf_mesh_bvh_closest into sentinel-padded buffers -> dict of arrays without the (checked) padding"""
    from customnerf_amd._lib import lib, check, ptr, stream
    ws, nbytes, _, V, F = tree
    Q = len(pts)
    gp = cuda(np.asarray(pts, np.float32))
    d2 = torch.full((Q + PAD,), SENTINEL, device="cuda")
    face = torch.full((Q + PAD,), int(SENTINEL), dtype=torch.int32, device="cuda")
    point = torch.full((3 * Q + PAD,), SENTINEL, device="cuda") if "point" in want else None
    bary = torch.full((3 * Q + PAD,), SENTINEL, device="cuda") if "bary" in want else None
    stats = torch.zeros(2 + PAD, dtype=torch.int64, device="cuda") if "stats" in want else None
    p = lambda t: None if t is None else ptr(t)                                   # noqa: E731
    check(lib.cnerf_mesh_bvh_closest(ptr(ws), nbytes, V, F, ptr(gp) if Q else None, Q, ptr(d2), ptr(face), p(point), p(bary), p(stats), stream()),
          "closest")
    out = {'dist2': d2.cpu().numpy(), 'face': face.cpu().numpy()}
    assert (out['dist2'][Q:] == SENTINEL).all() and (out['face'][Q:] == int(SENTINEL)).all()
    out['dist2'], out['face'] = out['dist2'][:Q], out['face'][:Q]
    for k, t in (("point", point), ("bary", bary)):
        if t is not None:
            a = t.cpu().numpy()
            assert (a[3 * Q:] == SENTINEL).all()
            out[k] = a[:3 * Q].reshape(Q, 3)
    if stats is not None:
        s = stats.cpu().numpy()
        assert (s[2:] == 0).all()
        out['stats'] = (int(s[0]), int(s[1]))
    return out


def assert_same_closest(got, want):
    np.testing.assert_array_equal(got['face'], want['face'])
    for k in ('dist2', 'point', 'bary'):
        if k in got:
            np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)


@pytest.mark.parametrize("name,v,f", MESHES, ids=[m[0] for m in MESHES])
def test_closest_matches_brute_force(name, v, f):
    """dist2, face, point and bary bit-equal to the brute-force restatement; the counts; outputs without point / bary the same; padding
    untouched"""
    ok, flags = B.participating(v, f)
    tree = gpu_build(v, f)
    assert tree[2][0] == ok.sum() and tree[2][1] == flags
    pts = queries(v, f)
    want = B.closest(v, f, pts)
    got = gpu_closest(tree, pts)
    assert_same_closest(got, want)
    assert (want['face'][-4:] == -1).all() and np.isinf(want['dist2'][-4:]).all()
    if ok.any():
        assert (want['face'][:-4] >= 0).all() and ok[want['face'][:-4]].all()
        ties = sum(int((B.point_triangles(p, *(v[f[ok][:, k]] for k in range(3)))[0] == d).sum() > 1) for p, d in zip(pts[:-4:7], want['dist2'][:-4:7]))
        print(f"{name}: {len(pts)} queries over {int(ok.sum())} faces, {ties} of {len(pts[:-4:7])} probed queries tie between faces, "
              f"{got['stats'][1] / len(pts):.1f} triangle tests and {got['stats'][0] / len(pts):.1f} box tests per query")
    else:
        assert (want['face'] == -1).all() and got['stats'] == (0, 0)
    assert_same_closest(gpu_closest(tree, pts, want=()), want)
    assert_same_closest(gpu_closest(tree, pts[:0]), B.closest(v, f, pts[:0]))


def test_realistic_size():
    """a marching-cubes sphere that fills a 128^3 lattice, extracted on the device (146 k faces; a sphere inside 128^3 has at most about
    150 k): 512 queries bit-equal to brute force"""
    from customnerf_amd import mesh
    (X, Y, Z), sp = lattice((128, 128, 128), -1.0, 1.0)
    vol = (0.98 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)
    gv, gf, _ = mesh.marching_cubes(cuda(vol), 0.0, spacing=sp, origin=(-1.0, -1.0, -1.0))
    v, f = gv.cpu().numpy(), gf.cpu().numpy()
    assert 140_000 < len(f) < 160_000
    rng = np.random.default_rng(4)
    d = rng.standard_normal((512, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([rng.normal(0.98, 0.02, 384), rng.uniform(0.0, 0.5, 64), rng.uniform(1.5, 50.0, 64)])
    pts = (d * r[:, None]).astype(np.float32)
    pts[:64] = v[rng.integers(0, len(v), 64)]                                     # vertices: ties between their faces
    bvh = mesh.build_bvh(gv, gf)
    assert bvh.n_faces == len(f) and not bvh.bad_index and not bvh.non_finite
    got = mesh.closest_point(bvh, cuda(pts), want_point=True, want_bary=True, want_stats=True)
    want = B.closest(v, f, pts)
    assert_same_closest({k: got[k].cpu().numpy() for k in ('dist2', 'face', 'point', 'bary')}, want)
    print(f"{len(f)} faces: {got['stats'][1] / 512:.1f} triangle tests and {got['stats'][0] / 512:.1f} box tests per query")
    assert got['stats'][1] / 512 < len(f) / 16


def gpu_sample(v, f, spacing, max_samples=None):
    """the C sampler into sentinel-padded buffers -> (dict of arrays, total, flags)"""
    from customnerf_amd._lib import lib, check, ptr, stream
    gv, gf = cuda(np.asarray(v, np.float32)), cuda(np.asarray(f, np.int32))
    V, F = len(v), len(f)
    need = C.c_uint64(0)
    check(lib.cnerf_mesh_sample_workspace_bytes(F, C.byref(need)), "sample_ws")
    ws = torch.full((need.value + 256,), 0x5a, dtype=torch.uint8, device="cuda")
    counts = torch.full((2 + PAD,), 0x55, dtype=torch.int64, device="cuda")
    pv, pf = (ptr(gv) if V else None), (ptr(gf) if F else None)
    check(lib.cnerf_mesh_sample_count(pv, V, pf, F, spacing, ptr(ws), need.value, ptr(counts), stream()), "sample_count")
    c = counts.cpu().numpy()
    assert (c[2:] == 0x55).all()
    total, flags = int(c[0]), int(c[1])
    n = total if max_samples is None else min(total, max_samples)
    pts = torch.full((3 * n + PAD,), SENTINEL, device="cuda")
    face = torch.full((n + PAD,), int(SENTINEL), dtype=torch.int32, device="cuda")
    bary = torch.full((3 * n + PAD,), SENTINEL, device="cuda")
    w = torch.full((n + PAD,), SENTINEL, device="cuda")
    check(lib.cnerf_mesh_sample_emit(pv, V, pf, F, spacing, ptr(ws), need.value, ptr(pts), ptr(face), ptr(bary), ptr(w), n, stream()), "sample_emit")
    torch.cuda.synchronize()
    assert (ws[need.value:] == 0x5a).all()
    out = {k: t.cpu().numpy() for k, t in dict(points=pts, face=face, bary=bary, weight=w).items()}
    for k, m in (("points", 3), ("face", 1), ("bary", 3), ("weight", 1)):
        assert (out[k][m * n:] == (int(SENTINEL) if k == "face" else SENTINEL)).all(), k
        out[k] = out[k][:m * n].reshape((n, 3) if m == 3 else (n,))
    return out, total, flags


@pytest.mark.parametrize("name,v,f", MESHES, ids=[m[0] for m in MESHES])
def test_sampler_matches_restatement(name, v, f):
    lo, hi = finite_box(v, f)
    diag = float(np.linalg.norm(hi.astype(np.float64) - lo)) or 1.0
    for spacing in (0.3 * diag, 0.02 * diag, 0.004 * diag):
        spacing = float(np.float32(spacing))
        want = B.sample(v, f, spacing)
        got, total, flags = gpu_sample(v, f, spacing)
        assert total == want['total'] and flags == want['flags']
        np.testing.assert_array_equal(got['face'], want['face'])
        for k in ('points', 'bary', 'weight'):
            np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
        # max_samples: the first samples only, nothing after them
        cut = total // 3
        part, total2, _ = gpu_sample(v, f, spacing, max_samples=cut)
        assert total2 == total and len(part['face']) == cut
        np.testing.assert_array_equal(part['points'].view(np.uint32), want['points'][:cut].view(np.uint32))
        np.testing.assert_array_equal(part['face'], want['face'][:cut])
    print(f"{name}: {total} samples at the finest spacing")


def test_sampler_clamp_and_python():
    from customnerf_amd import mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [1000, 0, 0], [0, 1000, 0]], np.float32)
    f = np.array([[0, 1, 2], [3, 3, 3], [0, 4, 5]], np.int32)
    want = B.sample(v, f, 0.5)
    got, total, flags = gpu_sample(v, f, 0.5)
    assert flags == 4 == want['flags'] and total == 4 + 1 + 65536 == want['total']
    for k in ('points', 'bary', 'weight'):
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
    assert got['weight'][4] == 0 and np.array_equal(got['points'][4], [2, 2, 2])
    with pytest.raises(ValueError, match="256"):
        mesh.sample_surface(cuda(v), cuda(f), 0.5)
    pts, face, bary, w = mesh.sample_surface(cuda(v), cuda(f[:2]), 0.5)
    np.testing.assert_array_equal(pts.cpu().numpy().view(np.uint32), want['points'][:5].view(np.uint32))
    assert face.tolist() == [0, 0, 0, 0, 1] and tuple(bary.shape) == (5, 3) and w.dtype == torch.float32
    with pytest.raises(ValueError, match="max_samples"):
        mesh.sample_surface(cuda(v), cuda(f[:2]), 0.5, max_samples=4)
    for sp in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="spacing"):
            mesh.sample_surface(cuda(v), cuda(f), sp)
    pts, face, bary, w = mesh.sample_surface(cuda(v), cuda(f[:0]), 0.5)
    assert tuple(pts.shape) == (0, 3) and tuple(w.shape) == (0,)


@pytest.mark.parametrize("name", ["sphere", "two_tori", "bad_faces"])
def test_two_runs_are_identical(name):
    """build and query twice into fresh buffers: every byte of the workspace (header, records, boxes and the sort's scratch; what the build
    does not write keeps the fill) and every output"""
    _, v, f = next(m for m in MESHES if m[0] == name)
    pts = queries(v, f, seed=5)
    runs = []
    for _ in range(2):
        tree = gpu_build(v, f)
        out = gpu_closest(tree, pts)
        runs.append((tree[0].cpu().numpy(), tree[2], out))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    for k in ('dist2', 'face', 'point', 'bary'):
        np.testing.assert_array_equal(runs[0][2][k].view(np.uint32), runs[1][2][k].view(np.uint32))
    assert runs[0][2]['stats'] == runs[1][2]['stats']
    # and the fill does not leak into the result
    other = gpu_closest(gpu_build(v, f, fill=0xa7), pts)
    for k in ('dist2', 'face', 'point', 'bary'):
        np.testing.assert_array_equal(other[k].view(np.uint32), runs[0][2][k].view(np.uint32))


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_tree_prunes(name):
    """surface samples moved by 2 % of the diagonal: fewer than F / 16 triangle tests per query (a traversal that prunes nothing makes F).
    Measured on an MI355X (also in DESIGN.md 4c): sphere 71.5 triangle tests per query (F / 161) and 190.1 box tests, torus 60.7 (F / 120)
    and 147.4."""
    _, v, f = next(m for m in MESHES if m[0] == name)
    lo, hi = finite_box(v, f)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(2)
    s = B.sample(v, f, 0.02 * diag)['points']
    pts = (s + rng.standard_normal(s.shape) * 0.02 * diag).astype(np.float32)
    got = gpu_closest(gpu_build(v, f), pts, want=("stats",))
    per = got['stats'][1] / len(pts)
    print(f"{name}: F = {len(f)}, {len(pts)} queries, {per:.1f} triangle tests (F / {len(f) / per:.0f}) and {got['stats'][0] / len(pts):.1f} box tests per query")
    assert per < len(f) / 16
    sub = rng.permutation(len(pts))[:64]
    np.testing.assert_array_equal(got['dist2'][sub].view(np.uint32), B.closest(v, f, pts[sub])['dist2'].view(np.uint32))


def assert_same_report(got, want):
    for way in ('a_to_b', 'b_to_a'):
        assert (way in got) == (way in want)
        if way not in want:
            continue
        g, w = got[way], want[way]
        assert g['max'] == w['max'] and g['max_point'] == w['max_point'] and g['max_face'] == w['max_face'] and g['n_samples'] == w['n_samples']
        for k in ('mean', 'rms'):
            print(f"{way} {k}: {g[k]!r} against {w[k]!r}")
            assert abs(g[k] - w[k]) <= 1e-9 * abs(w[k])
    assert got['hausdorff'] == want['hausdorff']


def test_distance_matches_restatement():
    from customnerf_amd import mesh
    v, f = sphere_mesh(24, 0.7)
    dv, df, _, _ = (t.cpu().numpy() if t is not None else None for t in mesh.decimate(cuda(v), cuda(f), 600))
    for kw in (dict(), dict(symmetric=False), dict(include_vertices=False)):
        got = mesh.distance(cuda(dv), cuda(df), cuda(v), cuda(f), spacing=0.06, **kw)
        want = B.distance(dv, df, v, f, 0.06, **kw)
        assert_same_report(got, want)
        assert got['spacing'] == 0.06 and 0 < got['hausdorff'] < 0.1
    # the default spacing: 0.002 x the diagonal of the box around both
    got = mesh.distance(cuda(dv), cuda(df), cuda(v), cuda(f), symmetric=False, include_vertices=False)
    both = np.concatenate([dv, v])
    want_sp = 0.002 * float(np.linalg.norm((both.max(0) - both.min(0)).astype(np.float64)))
    assert abs(got['spacing'] - want_sp) <= 1e-12 * want_sp
    assert got['a_to_b']['n_samples'] == B.sample(dv, df, got['spacing'])['total']
    with pytest.raises(ValueError):
        mesh.distance(cuda(dv), cuda(df), cuda(v), cuda(f[:0]))
    with pytest.raises(ValueError):
        mesh.distance(cuda(dv), cuda(df), cuda(v), cuda(f), spacing=0.0)


def test_distance_exact_and_translate():
    from customnerf_amd import mesh
    v, f = grid(16)
    v2 = v + np.array([0, 0, 0.25], np.float32)
    d = mesh.distance(cuda(v), cuda(f), cuda(v2), cuda(f), spacing=0.4)
    for way in ('a_to_b', 'b_to_a'):
        assert d[way]['max'] == d[way]['mean'] == d[way]['rms'] == 0.25 and d[way]['n_samples'] > 2 * len(f)
    assert d['hausdorff'] == 0.25
    # a closed mesh against its own translate by t: every point p of A has p + t in B, so each one-sided distance is at most |t|
    sv, sf = sphere_mesh(24, 0.7)
    t = np.array([0.03, -0.02, 0.05], np.float32)
    d = mesh.distance(cuda(sv), cuda(sf), cuda(sv + t), cuda(sf))
    norm = float(np.linalg.norm(t.astype(np.float64)))
    print(f"hausdorff {d['hausdorff']!r} against |t| = {norm!r}")
    assert 0.5 * norm < d['hausdorff'] <= norm * (1 + 1e-5)
    assert 0 < d['a_to_b']['mean'] <= d['a_to_b']['rms'] <= d['a_to_b']['max']


def test_distance_accepts_large_faces():
    """a 12-triangle cube at the default spacing needs k = 289 > 256 per face: distance() samples those faces at k = 256 (sample_surface
    itself still refuses); against the same cube moved by t along x every one-sided distance is at most |t|, and the far side reaches it"""
    from customnerf_amd import mesh
    c = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                 np.int32)
    with pytest.raises(ValueError, match="256"):
        mesh.sample_surface(cuda(c), cuda(f), 0.002 * math.sqrt(3.0))
    d = mesh.distance(cuda(c), cuda(f), cuda(c + np.array([0.25, 0, 0], np.float32)), cuda(f))
    assert d['a_to_b']['n_samples'] == 12 * 65536 and d['hausdorff'] == 0.25
    # mean over the six unit faces: x = 0 is 0.25 away; a side lies in the other cube's side except a strip 0.25 wide: 0.25^2 / 2; the
    # x = 1 face is inside the other cube, min(0.25, distance to its border) away: 0.5^2 * 0.25 + 1 / 12.  The centroid rule is exact where
    # the distance is linear over a sub-triangle; the others (a few per cent, crossed by a kink) err by less than their diameter 0.0055
    want = (0.25 + 4 * 0.03125 + (0.0625 + 1.0 / 12)) / 6
    print(f"mean {d['a_to_b']['mean']!r} against {want!r}")
    assert abs(d['a_to_b']['mean'] - want) < 1e-3


def test_extract_mesh_deviation(dtype_guard):
    """the report of extract_mesh(deviation=True) equals mesh.distance called by hand on the result and on an undecimated extraction"""
    from customnerf_amd import mesh
    model = gaussian_model(dtype_guard, False)
    kw = dict(resolution=64, threshold=10.0, aabb=AABB, keep_largest=True)
    base = model.extract_mesh(**kw)
    assert 'deviation' not in base
    assert model.extract_mesh(deviation=True, **kw)['deviation'] is None          # no lossy pass ran
    m = model.extract_mesh(target_faces=800, deviation=True, **kw)
    dev = m['deviation']
    step = 1.0 / 63
    assert len(dev['step']) == 3 and all(abs(s - step) < 1e-6 for s in dev['step'])
    assert torch.equal(model.extract_mesh(target_faces=800, **kw)['verts'], m['verts'])
    by_hand = mesh.distance(m['verts'], m['faces'], base['verts'], base['faces'], spacing=0.5 * min(dev['step']))
    assert {k: v for k, v in dev.items() if k != 'step'} == by_hand
    print(f"decimated to {m['faces'].shape[0]} of {base['faces'].shape[0]} faces: hausdorff {dev['hausdorff'] / step:.3f} voxels, "
          f"rms {dev['a_to_b']['rms'] / step:.4f} / {dev['b_to_a']['rms'] / step:.4f} voxels")
    for way in ('a_to_b', 'b_to_a'):
        assert 0 < dev[way]['mean'] <= dev[way]['rms'] <= dev[way]['max'] < R_SPHERE and dev[way]['n_samples'] > 0
    assert 0 < dev['hausdorff'] < R_SPHERE
    for opt in (dict(smooth=5), dict(simplify=3)):
        d = model.extract_mesh(deviation=True, deviation_spacing=0.01, **opt, **kw)['deviation']
        assert d['spacing'] == 0.01 and math.isfinite(d['hausdorff']) and 0 < d['hausdorff'] < R_SPHERE
        assert all(math.isfinite(d[w][k]) and d[w][k] > 0 for w in ('a_to_b', 'b_to_a') for k in ('max', 'mean', 'rms'))
