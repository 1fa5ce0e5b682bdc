"""GPU: ray queries through the mesh BVH (csrc/mesh_bvh.hip, k_bvh_raycast / k_bvh_occluded) and the ambient occlusion built on them,
against their NumPy restatement (tests/ray_restatement.py): t, face, bary and the any-hit bit bit-equal to brute force over hand-made and
marching-cubes meshes for the three cull modes; watertightness on the device; any-hit against closest-hit; pruning; two runs identical;
agreement with the rasteriser; ambient occlusion; extract_mesh(ao=) / save_mesh end to end; validation."""
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
import mc_restatement as R  # noqa: E402
import ray_restatement as RR  # noqa: E402
import ray_testlib as T  # noqa: E402
from mesh_testlib import AABB, cuda, dtype_guard, gaussian_model  # noqa: E402,F401

SENTINEL = -7.0
PAD = 8
CULLS = ('none', 'back', 'front')
INSIDE = np.array([0.013, -0.021, 0.017], np.float32)


def gpu_build(v, f, fill=0x5a):
    """cnerf_mesh_bvh_build into an over-allocated workspace -> (ws tensor, nbytes, V, F)"""
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib, check, ptr, stream
    gv, gf = cuda(np.asarray(v, np.float32)), cuda(np.asarray(f, np.int32))
    V, F = len(v), len(f)
    nbytes = mesh.bvh_workspace_bytes(V, F)
    ws = torch.full((nbytes + 256,), fill, dtype=torch.uint8, device="cuda")
    counts = torch.empty(2, dtype=torch.int32, device="cuda")
    check(lib.cnerf_mesh_bvh_build(ptr(gv) if V else None, V, ptr(gf) if F else None, F, ptr(ws), nbytes, ptr(counts), stream()), "build")
    return ws, nbytes, V, F


def _range(x, Q):
    """(scalar, tensor or None) of a t_min / t_max given as a number or a [Q] array"""
    if np.ndim(x) == 0:
        return float(x), None
    return 0.0, torch.cat([cuda(np.asarray(x, np.float32)), torch.full((PAD,), SENTINEL, device="cuda")])


def gpu_cast(tree, o, d, tmin=0.0, tmax=np.inf, cull='none', want=("t", "face", "bary", "stats")):
    """cnerf_mesh_bvh_raycast into sentinel-padded buffers -> dict of arrays without the (checked) padding; the workspace is checked too"""
    from customnerf_amd._lib import lib, check, ptr, stream
    ws, nbytes, V, F = tree
    before = ws.clone()
    Q = len(o)
    go, gd = cuda(np.asarray(o, np.float32)), cuda(np.asarray(d, np.float32))
    (t0, p0), (t1, p1) = _range(tmin, Q), _range(tmax, Q)
    t = torch.full((Q + PAD,), SENTINEL, device="cuda") if "t" in want else None
    face = torch.full((Q + PAD,), int(SENTINEL), dtype=torch.int32, device="cuda") if "face" in want else None
    bary = torch.full((3 * Q + PAD,), SENTINEL, device="cuda") if "bary" in want else None
    stats = torch.zeros(2 + PAD, dtype=torch.int64, device="cuda") if "stats" in want else None
    p = lambda x: None if x is None else ptr(x)                                   # noqa: E731
    check(lib.cnerf_mesh_bvh_raycast(ptr(ws), nbytes, V, F, ptr(go) if Q else None, ptr(gd) if Q else None, Q, t0, t1, p(p0), p(p1),
                                     RR.CULL[cull], p(t), p(face), p(bary), p(stats), stream()), "raycast")
    torch.cuda.synchronize()
    assert torch.equal(ws, before)                                                # a query writes nothing into the tree or past it
    out = {}
    for k, buf, m, s in (("t", t, 1, SENTINEL), ("face", face, 1, int(SENTINEL)), ("bary", bary, 3, SENTINEL)):
        if buf is not None:
            a = buf.cpu().numpy()
            assert (a[m * Q:] == s).all(), k
            out[k] = a[:m * Q].reshape((Q, 3) if m == 3 else (Q,))
    if stats is not None:
        s = stats.cpu().numpy()
        assert (s[2:] == 0).all()
        out['stats'] = (int(s[0]), int(s[1]))
    return out


def gpu_occluded(tree, o, d, tmin=0.0, tmax=np.inf, cull='none'):
    """cnerf_mesh_bvh_occluded into a sentinel-padded buffer -> (bool [Q], stats)"""
    from customnerf_amd._lib import lib, check, ptr, stream
    ws, nbytes, V, F = tree
    Q = len(o)
    go, gd = cuda(np.asarray(o, np.float32)), cuda(np.asarray(d, np.float32))
    (t0, p0), (t1, p1) = _range(tmin, Q), _range(tmax, Q)
    occ = torch.full((Q + PAD,), 0x5a, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(2 + PAD, dtype=torch.int64, device="cuda")
    p = lambda x: None if x is None else ptr(x)                                   # noqa: E731
    check(lib.cnerf_mesh_bvh_occluded(ptr(ws), nbytes, V, F, ptr(go) if Q else None, ptr(gd) if Q else None, Q, t0, t1, p(p0), p(p1),
                                      RR.CULL[cull], ptr(occ), ptr(stats), stream()), "occluded")
    a, s = occ.cpu().numpy(), stats.cpu().numpy()
    assert (a[Q:] == 0x5a).all() and (s[2:] == 0).all() and set(np.unique(a[:Q])) <= {0, 1}
    return a[:Q] != 0, (int(s[0]), int(s[1]))


def assert_same_cast(got, want):
    np.testing.assert_array_equal(got['face'], want['face'])
    for k in ('t', 'bary'):
        if k in got:
            np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)


@pytest.mark.parametrize("name", [m[0] for m in T.MESHES])
def test_cast_matches_brute_force(name):
    """t, face, bary and the any-hit bit bit-equal to the brute-force restatement for the mixed batch with per-ray ranges, in the three cull
    modes; outputs without bary the same; any-hit == (face >= 0) and tests no more triangles; t_max at a hit's own t hits, one float below
    misses; the degenerate rays miss; ray counts 0, 1, 65, 257 with a scalar range; padding and workspace untouched"""
    v, f = T.mesh(name)
    b = T.batch(name)
    o, d, tmin, tmax, want = b['o'], b['d'], b['tmin'], b['tmax'], b['want']
    tree = gpu_build(v, f)
    for cull in CULLS:
        got = gpu_cast(tree, o, d, tmin, tmax, cull)
        assert_same_cast(got, want[cull])
        occ, ostats = gpu_occluded(tree, o, d, tmin, tmax, cull)
        np.testing.assert_array_equal(occ, want[cull]['occluded'])
        np.testing.assert_array_equal(occ, got['face'] >= 0)
        assert ostats[1] <= got['stats'][1] and ostats[0] <= got['stats'][0]
        assert (got['face'][-T.N_DEGENERATE:] == -1).all() and np.isposinf(got['t'][-T.N_DEGENERATE:]).all() and not occ[-T.N_DEGENERATE:].any()
        assert_same_cast(gpu_cast(tree, o, d, tmin, tmax, cull, want=("t", "face")), want[cull])
        print(f"{name} cull={cull}: {len(o)} rays over {len(f)} faces, {int(occ.sum())} hit, {got['stats'][1] / len(o):.1f} triangle and "
              f"{got['stats'][0] / len(o):.1f} box tests per ray (any-hit {ostats[1] / len(o):.1f} and {ostats[0] / len(o):.1f})")
    got = gpu_cast(tree, o, d, tmin, tmax, 'none')
    if len(b['at_t']):
        np.testing.assert_array_equal(got['face'][b['at_t']], b['first_face'])
        np.testing.assert_array_equal(got['t'][b['at_t']].view(np.uint32), b['first_t'].view(np.uint32))
        assert (got['face'][b['below_t']] == -1).all()
    assert len(b['at_t']) > 100 or name in ("F0", "F1", "F4", "F5", "F13")
    if name == "F0":
        assert (got['face'] == -1).all() and got['stats'] == (0, 0)
    # a scalar range, ray counts around the wave and the block
    lo, hi = np.float32(0.25), np.float32(2.0)
    ref = RR.cast(v, f, o[:257], d[:257], lo, hi, culls=('none',))['none']
    for Q in (0, 1, 65, 257):
        got = gpu_cast(tree, o[:Q], d[:Q], lo, hi)
        assert_same_cast(got, {k: ref[k][:Q] for k in ('t', 'face', 'bary')})
        occ, _ = gpu_occluded(tree, o[:Q], d[:Q], lo, hi)
        np.testing.assert_array_equal(occ, ref['occluded'][:Q])
    assert name == "F0" or 0 < ref['occluded'].sum() < 257


def watertight_sets():
    iv, if_ = T.icosphere(2)
    yield "icosphere_centre", iv, if_, np.zeros(3, np.float32)
    yield "icosphere", iv, if_, INSIDE
    sv, sf = T.mesh("sphere")
    yield "mc_sphere", sv, sf, INSIDE


@pytest.mark.parametrize("name,v,f,origin", list(watertight_sets()), ids=[w[0] for w in watertight_sets()])
def test_watertight_on_device(name, v, f, origin):
    """every vertex, edge midpoint and face centroid of a closed mesh, aimed at from inside: every ray hits, at the target (the
    marching-cubes sphere is not exactly convex: a face in front of the target's may be met first)"""
    from customnerf_amd import mesh
    tg = T.targets(v, f)
    o, d = T.rays_to(origin, tg)
    bvh = mesh.build_bvh(cuda(v), cuda(f))
    got = mesh.ray_cast(bvh, cuda(o), cuda(d))
    occ = mesh.occluded(bvh, cuda(o), cuda(d))
    t, face = got['t'].cpu().numpy(), got['face'].cpu().numpy()
    print(f"{name}: {len(tg)} rays, {int((face < 0).sum())} misses, max |t - 1| = {np.abs(t - 1).max():.3g}")
    assert (face >= 0).all() and occ.all()
    # d = target - origin, so the target sits at t = 1.  On the convex icosphere that is the hit; the marching-cubes sphere (lattice step
    # h = 0.1, radius r = 0.9, zero-area and sliver faces where the sphere passes through lattice points) is a sheet within h^2 / (8 r) =
    # 1.4e-3 of the sphere, and the hit lies in that sheet
    assert np.abs(t - 1.0).max() <= (1e-2 if name == "mc_sphere" else 1e-5)


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_tree_prunes(name):
    """rays from outside: fewer than F / 16 triangle tests per ray (a traversal that prunes nothing makes F); the counts of two runs are equal"""
    v, f = T.mesh(name)
    b = T.batch(name)
    o, d = b['o'][:640], b['d'][:640]                                             # the batch's first group: from outside towards the box
    tree = gpu_build(v, f)
    runs = [gpu_cast(tree, o, d) for _ in range(2)]
    per = runs[0]['stats'][1] / len(o)
    print(f"{name}: F = {len(f)}, {len(o)} rays, {per:.1f} triangle tests (F / {len(f) / per:.0f}) and {runs[0]['stats'][0] / len(o):.1f} box "
          f"tests per ray")
    assert 0 < per < len(f) / 16
    assert runs[0]['stats'] == runs[1]['stats']
    occ = [gpu_occluded(tree, o, d) for _ in range(2)]
    assert occ[0][1] == occ[1][1] and 0 < occ[0][1][1] / len(o) < len(f) / 16


@pytest.mark.parametrize("name", ["sphere", "bad_faces"])
def test_two_runs_are_identical(name):
    """build and query twice into fresh buffers, and once more over another fill of the workspace: every output and the statistics"""
    v, f = T.mesh(name)
    b = T.batch(name)
    runs = []
    for fill in (0x5a, 0x5a, 0xa7):
        tree = gpu_build(v, f, fill=fill)
        runs.append((gpu_cast(tree, b['o'], b['d'], b['tmin'], b['tmax'], 'back'), gpu_occluded(tree, b['o'], b['d'], b['tmin'], b['tmax'], 'back')))
    for other in runs[1:]:
        for k in ('t', 'face', 'bary'):
            np.testing.assert_array_equal(other[0][k].view(np.uint32), runs[0][0][k].view(np.uint32))
        assert other[0]['stats'] == runs[0][0]['stats'] and other[1][1] == runs[0][1][1]
        np.testing.assert_array_equal(other[1][0], runs[0][1][0])


def test_agrees_with_rasteriser():
    """a 64 x 64 pinhole view of the (convex) sphere: where the rasteriser reports a face and the pixel is interior to it (smallest
    barycentric >= 0.01), the ray through the pixel hits the same face at the same camera-axis depth within 1e-4; empty pixels whose ray
    passes the sphere's bounding radius miss.  The camera is a long lens (distance 100, focal length 2000 pixels: the sphere is 18 pixels
    in radius): the rasteriser snaps projected vertices to 1 / 256 pixel, which moves its plane at a pixel centre by up to sqrt(2) / 512
    pixel, a relative depth of (sqrt(2) / 512) tan(theta) / f for a face seen at the angle theta from head-on — 1.4e-6 tan(theta) at
    f = 2000, below the 1e-4 asked for up to theta = 89.2 degrees, where at f = 69 (a 50 degree lens at distance 3.5, measured: 6.3e-4 at
    the limb) it is 4e-5 tan(theta).  The ray cast has no such step: its depth is the plane's to a few 1e-7."""
    from customnerf_amd import mesh, scene
    from customnerf_amd.nerf.provider_utils import generate_rays
    v, f = T.mesh("sphere")
    H = W = 64
    c2w = np.asarray(scene.camera_pose(3, radius=100.0, elev_deg=20.0), np.float32)
    intr = (2000.0, 2000.0, W / 2.0, H / 2.0)
    gv, gf = cuda(v), cuda(f)
    vis = mesh.rasterize(gv, gf, c2w, intr, H, W, cull='back')
    ro, rd = generate_rays(cuda(c2w[None]), *intr, H, W)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    got = mesh.ray_cast(mesh.build_bvh(gv, gf), ro, rd, cull='back')
    rface, rdepth, rbary = vis['face'].cpu().numpy().ravel(), vis['depth'].cpu().numpy().ravel(), vis['bary'].cpu().numpy().reshape(-1, 3)
    face, t = got['face'].cpu().numpy(), got['t'].cpu().numpy().astype(np.float64)
    o64, d64 = ro.cpu().numpy().astype(np.float64), rd.cpu().numpy().astype(np.float64)
    covered = rface >= 0
    interior = covered & (rbary.min(1) >= 0.01)
    print(f"{int(covered.sum())} covered pixels, {int(interior.sum())} interior")
    assert covered.sum() > 200 and interior.sum() >= 0.8 * covered.sum()
    np.testing.assert_array_equal(face[interior], rface[interior])
    fwd = -c2w[:3, 2].astype(np.float64)                                          # the nerfstudio camera looks along -z
    depth = t[interior] * (d64[interior] @ fwd)
    rel = np.abs(depth - rdepth[interior]) / rdepth[interior]
    print(f"depth: max relative difference {rel.max():.3g}")
    assert rel.max() <= 1e-4
    along = (o64 * d64).sum(1) / (d64 * d64).sum(1)
    miss_by = np.linalg.norm(o64 - along[:, None] * d64, axis=1)                  # the ray's distance from the sphere's centre
    outside = ~covered & (miss_by > 0.9 * 1.01)
    assert outside.sum() > 200 and (face[outside] == -1).all()


def fetch_ao_rays(v, n, K, bias):
    from customnerf_amd import mesh
    org, d = mesh.ao_rays(cuda(v), cuda(n), mesh.ao_directions(K), bias)
    return org.contiguous().cpu().numpy(), d.contiguous().cpu().numpy()


def test_ambient_occlusion_matches_restatement():
    """the torus (it shadows itself) with rays made on the device: the escaped counts of the brute force are equalled exactly, whatever
    the chunk; the device's rays are the restatement's up to rounding; an unused vertex gets 1"""
    from customnerf_amd import mesh
    v, f = T.mc_torus((20, 18, 12))                                               # about 900 faces: the brute force stays quick
    v = np.concatenate([v, [[5.0, 5.0, 5.0]]]).astype(np.float32)                 # a vertex no face uses
    K, bias = 16, 1e-3
    gv, gf = cuda(v), cuda(f)
    n = mesh.vertex_normals(gv, gf)
    n[-1] = torch.tensor([0.0, 0.0, 1.0])
    org, d = fetch_ao_rays(v, n.cpu().numpy(), K, bias)
    want, free = RR.ambient_occlusion(v, f, org, d, radius=0.8)
    for chunk in (2 ** 22, 1000):
        got = mesh.ambient_occlusion(gv, gf, normals=n, samples=K, radius=0.8, bias=bias, chunk=chunk).cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    sv, sf = (cuda(x) for x in T.mesh("F13"))                                     # a chunk smaller than K splits the directions too
    assert torch.equal(mesh.ambient_occlusion(sv, sf, samples=K, chunk=7), mesh.ambient_occlusion(sv, sf, samples=K))
    assert want[-1] == 1.0 and 0.3 < want[:-1].mean() < 0.98 and (free[:-1] < K).sum() > len(v) // 8
    ro, rd = RR.ao_rays(v, n.cpu().numpy(), K, bias)
    assert np.abs(ro - org).max() <= 1e-6 and np.abs(rd - d).max() <= 1e-6
    np.testing.assert_array_equal(mesh.ao_directions(K).numpy().view(np.uint32), RR.ao_directions(K).view(np.uint32))
    # without normals and with the default bias and radius: vertex_normals and 1e-4 of the box diagonal
    got = mesh.ambient_occlusion(gv[:-1], gf, samples=K).cpu().numpy()
    diag = float(np.linalg.norm((v[:-1].max(0) - v[:-1].min(0)).astype(np.float64)))
    org, d = fetch_ao_rays(v[:-1], n[:-1].cpu().numpy(), K, 1e-4 * diag)
    np.testing.assert_array_equal(got, RR.ambient_occlusion(v[:-1], f, org, d)[0])


def test_ambient_occlusion_convex_and_inverted():
    """outward normals on the convex sphere: nothing is occluded; the sphere turned inside out (faces and normals flipped): every ray is
    stopped, which holds only because no ray slips between two faces"""
    from customnerf_amd import mesh
    v, f = T.mc_sphere(20)                                                        # a lattice that no vertex falls on: no zero-area face
    gv, gf = cuda(v), cuda(f)
    n = mesh.vertex_normals(gv, gf)
    assert (mesh.ambient_occlusion(gv, gf, normals=n, samples=32) == 1.0).all()
    flipped = gf[:, [0, 2, 1]].contiguous()
    assert (mesh.ambient_occlusion(gv, flipped, normals=-n, samples=32) == 0.0).all()
    assert (mesh.ambient_occlusion(gv, flipped, samples=32) == 0.0).all()         # vertex_normals of the flipped faces point inwards


def test_ambient_occlusion_floor_and_wall():
    """a unit floor square, finely triangulated, with a wall of height 1 along its edge x = 0: dark at the wall's foot, open far from it
    within the radius, and non-decreasing with the distance from the wall"""
    from customnerf_amd import mesh
    n, K = 40, 64
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    floor = np.stack([i.ravel() / n, j.ravel() / n, np.zeros(i.size)], 1)
    wall = np.stack([np.zeros(i.size), j.ravel() / n, i.ravel() / n], 1)
    idx = lambda a, b: a * (n + 1) + b                                             # noqa: E731
    quads = np.array([[[idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)], [idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)]]
                      for a in range(n) for b in range(n)]).reshape(-1, 3)
    v = np.concatenate([floor, wall]).astype(np.float32)
    f = np.concatenate([quads, quads + len(floor)]).astype(np.int32)
    nrm = np.zeros_like(v)
    nrm[:len(floor), 2] = 1.0
    nrm[len(floor):, 0] = 1.0
    ao = mesh.ambient_occlusion(cuda(v), cuda(f), normals=cuda(nrm), samples=K, radius=0.5).cpu().numpy()
    fl = ao[:len(floor)].reshape(n + 1, n + 1)                                    # [x index, y index]
    x = np.arange(n + 1) / n
    inner = fl[:, n // 4:3 * n // 4 + 1]                                          # away from the wall's two ends
    print(f"floor AO by distance from the wall: {np.round(inner.mean(1)[::5], 3)}")
    assert (inner[x <= 0.05] < 0.75).all()
    assert (fl[x > 0.9] == 1.0).all()
    mid = fl[:, n // 2]
    assert (np.diff(mid) >= -2.0 / K).all() and mid[-1] == 1.0 and mid[0] < 0.75


def test_extract_mesh_ao_and_ply(dtype_guard, tmp_path):
    """extract_mesh(ao=K) adds 'ao' [V] in [0, 1] and changes nothing else; save_mesh writes it as grey unless color=True"""
    from customnerf_amd import mesh
    model = gaussian_model(dtype_guard, False)
    kw = dict(resolution=48, threshold=10.0, aabb=AABB)
    base = model.extract_mesh(**kw)
    assert 'ao' not in base and 'ao' not in model.extract_mesh(ao=0, **kw)
    m = model.extract_mesh(ao=32, **kw)
    V = m['verts'].shape[0]
    assert V > 100 and tuple(m['ao'].shape) == (V,) and m['ao'].dtype == torch.float32
    assert float(m['ao'].min()) >= 0.0 and float(m['ao'].max()) <= 1.0
    assert (m['ao'] == 1.0).float().mean() > 0.9                                  # a convex blob: open almost everywhere
    assert torch.equal(m['ao'], mesh.ambient_occlusion(m['verts'], m['faces'], normals=m['normals'], samples=32))
    for k, x in base.items():
        assert (m[k] is None and x is None) or (torch.equal(m[k], x) if torch.is_tensor(x) else m[k] == x), k
    path = str(tmp_path / "ao.ply")
    s = model.save_mesh(path, ao=32, **kw)
    ply = R.read_ply(path)
    grey = np.round(255.0 * s['ao'].cpu().numpy()).astype(np.uint8)
    np.testing.assert_array_equal(ply['colors'], np.repeat(grey[:, None], 3, 1))
    np.testing.assert_array_equal(ply['verts'], s['verts'].cpu().numpy())
    path2 = str(tmp_path / "colour.ply")
    c = model.save_mesh(path2, ao=32, color=True, **kw)
    np.testing.assert_array_equal(R.read_ply(path2)['colors'], c['colors'].cpu().numpy())
    assert 'ao' in c
    path3 = str(tmp_path / "plain.ply")
    model.save_mesh(path3, **kw)
    assert 'colors' not in R.read_ply(path3)
    with pytest.raises(ValueError, match="ao"):
        model.extract_mesh(ao=-1, **kw)


def test_validation():
    from customnerf_amd import mesh
    v, f = T.mesh("F13")
    gv, gf = cuda(v), cuda(f)
    bvh = mesh.build_bvh(gv, gf)
    o, d = torch.zeros(5, 3, device="cuda"), torch.ones(5, 3, device="cuda")
    for fn in (mesh.ray_cast, mesh.occluded):
        for args, kw in (((bvh, o.cpu(), d), {}), ((bvh, o, d.cpu()), {}), ((bvh, o[:, :2], d), {}), ((bvh, o, d[:4]), {}), ((bvh, o.ravel(), d), {}),
                         (("tree", o, d), {}), ((bvh, o, d), dict(cull='both')), ((bvh, o, d), dict(t_max=torch.ones(4, device="cuda"))),
                         ((bvh, o, d), dict(t_min=torch.zeros(5))), ((bvh, o.numpy(force=True), d), {})):
            with pytest.raises(ValueError):
                fn(*args, **kw)
    r = mesh.ray_cast(bvh, o, d, t_min=torch.zeros(5, device="cuda"), t_max=torch.full((5,), 9.0, device="cuda"), want_bary=True, want_stats=True)
    assert set(r) == {'t', 'face', 'bary', 'stats'} and r['t'].dtype == torch.float32 and r['face'].dtype == torch.int32
    assert mesh.occluded(bvh, o, d).dtype == torch.bool
    e = mesh.ray_cast(bvh, o[:0], d[:0], want_bary=True)
    assert tuple(e['t'].shape) == (0,) and tuple(e['bary'].shape) == (0, 3) and tuple(mesh.occluded(bvh, o[:0], d[:0]).shape) == (0,)
    for kw in (dict(samples=0), dict(samples=-3), dict(bias=float("nan")), dict(bias=float("inf")), dict(radius=0.0), dict(radius=-1.0),
               dict(radius=float("nan")), dict(chunk=0)):
        with pytest.raises(ValueError):
            mesh.ambient_occlusion(gv, gf, **kw)
    with pytest.raises(ValueError):
        mesh.ambient_occlusion(gv.cpu(), gf)
    with pytest.raises(ValueError):
        mesh.ambient_occlusion(gv, gf, normals=gv[:5])
    with pytest.raises(ValueError):
        mesh.ambient_occlusion(gv[:, :2], gf)
    with pytest.raises(ValueError):
        mesh.ao_directions(0)
    assert tuple(mesh.ambient_occlusion(gv, gf, samples=4, radius=math.inf).shape) == (len(v),)
    assert (mesh.ambient_occlusion(gv, gf[:0], samples=4) == 1.0).all()           # no face: nothing occludes
