"""GPU: brick-sparse marching cubes (csrc/mesh_sparse.hip, mesh.sparse_volume / marching_cubes_sparse) against the dense pass on the same
values — the same bits once the vertices are put in the dense order — against its NumPy restatement (tests/mc_sparse_restatement.py) in
its own order, the brick selection on analytic fields, and NeRFRenderer.extract_mesh(sparse=True) end to end."""
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
import mc_sparse_restatement as S  # noqa: E402
from mesh_testlib import AABB, dtype_guard, gaussian_model, host  # noqa: E402,F401

VOLUMES = S.volumes()
BITS = lambda a: np.ascontiguousarray(a).view(np.uint32)                        # noqa: E731


def assert_same_mesh(dense, sparse, normals=True):
    """dense (verts, faces, normals) == sparse (verts, faces, normals, keys) put in the dense order: vertices and normals bit for bit,
    faces as sorted row lists (table order within a cell is kept, so rows match without rotation)"""
    dv, df, dn = (t if isinstance(t, np.ndarray) else host(t) for t in dense)
    sv, sf, sn, keys = (host(t) for t in sparse)
    assert sv.shape == dv.shape and sf.shape == df.shape and len(np.unique(keys)) == len(keys)
    gv, gf, gn = S.reorder(sv, sf, sn, keys)
    np.testing.assert_array_equal(BITS(gv), BITS(dv))
    np.testing.assert_array_equal(gf, S.sorted_rows(df))
    if normals:
        np.testing.assert_array_equal(BITS(gn), BITS(dn))
    else:
        assert sn is None and dn is None


# ------------------------------------------------------------------------------------------------ 1. the kernels against the dense pass
@pytest.mark.parametrize("normals", [True, False], ids=["normals", "plain"])
@pytest.mark.parametrize("name, vol, level, sp, org", VOLUMES, ids=[v[0] for v in VOLUMES])
def test_sparse_equals_dense(name, vol, level, sp, org, normals):
    from customnerf_amd import mesh
    g = torch.from_numpy(vol).cuda()
    sv = mesh.sparse_volume_from_dense(g, level, spacing=sp, origin=org)
    assert sv.shape == vol.shape and sv.probe == 1 and sv.values.shape == (sv.n_bricks, 512) and sv.nbr.shape == (sv.n_bricks, 27)
    dense = mesh.marching_cubes(g, level, spacing=sp, origin=org, normals=normals)
    sparse = mesh.marching_cubes_sparse(sv, level, normals=normals, want_keys=True)
    assert len(dense[1]) > 0 and len(mesh.marching_cubes_sparse(sv, level, normals=normals)) == 3
    assert_same_mesh(dense, sparse, normals)


# ------------------------------------------------------------------------------------------------ 2. against the restatement, native order
@pytest.mark.parametrize("k", [0, 3], ids=[VOLUMES[0][0], VOLUMES[3][0]])
def test_sparse_matches_restatement(k):
    from customnerf_amd import mesh
    name, vol, level, sp, org = VOLUMES[k]
    ref_sel = S.select(vol, level, probe=1)
    sv = mesh.sparse_volume_from_dense(torch.from_numpy(vol).cuda(), level, spacing=sp, origin=org)
    np.testing.assert_array_equal(host(sv.coords), ref_sel["coords"])
    np.testing.assert_array_equal(host(sv.nbr), ref_sel["nbr"])
    assert sv.rounds == ref_sel["rounds"]
    inside = S.tiles(ref_sel["values"], ref_sel["coords"], ref_sel["nbr"], vol.shape)[2][:, 1:9, 1:9, 1:9].reshape(-1, 512)
    np.testing.assert_array_equal(BITS(host(sv.values))[inside], BITS(ref_sel["values"])[inside])      # where the lattice has a point
    ref = S.marching_cubes(ref_sel["values"], ref_sel["coords"], ref_sel["nbr"], vol.shape, level, sp, org)
    v, f, n, keys = (host(t) for t in mesh.marching_cubes_sparse(sv, level, want_keys=True))
    np.testing.assert_array_equal(keys, ref["keys"])
    np.testing.assert_array_equal(f, ref["faces"])
    np.testing.assert_array_equal(BITS(v), BITS(ref["verts"]))
    np.testing.assert_array_equal(BITS(n), BITS(ref["normals"]))             # correctly rounded sqrt and divisions on both sides
    st = torch.empty(sv.n_bricks, dtype=torch.uint8, device="cuda")
    from customnerf_amd._lib import lib, check, ptr, stream
    nbytes = mesh.sparse_workspace_bytes(sv.n_bricks)
    ws, counts = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    check(lib.cnerf_marching_cubes_sparse_count(ptr(sv.values), ptr(sv.coords), ptr(sv.nbr), sv.n_bricks, *vol.shape, level, ptr(ws), nbytes,
                                                ptr(st), ptr(counts), stream()), "count")
    np.testing.assert_array_equal(host(st), S.state(ref_sel["values"], ref_sel["coords"], ref_sel["nbr"], vol.shape, level))
    assert host(counts).tolist() == [len(v), len(f), 0]


# ------------------------------------------------------------------------------------------------ 3. selection on analytic fields
def sphere_fn(x):
    return 0.3 - torch.sqrt((x * x).sum(1))


def torus_fn(x):
    q = torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) - 0.3
    return 0.1 - torch.sqrt(q * q + x[:, 2] * x[:, 2])


def dense_of(fn, R):
    """fn on the full R^3 lattice of [-0.5, 0.5]^3, at the positions sparse_volume asks for: origin + ijk.float() * spacing in float32"""
    org = torch.full((3,), -0.5, device="cuda")
    sp = torch.full((3,), 1.0 / (R - 1), dtype=torch.float32, device="cuda")
    vol = torch.empty(R ** 3, device="cuda")
    for s in range(0, R ** 3, 2 ** 21):
        i = torch.arange(s, min(s + 2 ** 21, R ** 3), device="cuda", dtype=torch.int64)
        ijk = torch.stack([i // (R * R), (i // R) % R, i % R], dim=1)
        vol[s:s + len(i)] = fn((org + ijk.float() * sp).contiguous())
    return vol.view(R, R, R), org.tolist(), sp.tolist()


@functools.lru_cache(maxsize=None)
def analytic(which, R):
    """(dense volume, origin, spacing, the dense mesh on the host), computed once and left unchanged"""
    from customnerf_amd import mesh
    vol, org, sp = dense_of(sphere_fn if which == "sphere" else torus_fn, R)
    return vol, org, sp, tuple(host(t) for t in mesh.marching_cubes(vol, 0.0, spacing=sp, origin=org))


@pytest.mark.parametrize("which", ["sphere", "torus"])
def test_selection_96(which):
    from customnerf_amd import mesh
    vol, org, sp, dense = analytic(which, 96)
    sv = mesh.sparse_volume(sphere_fn if which == "sphere" else torus_fn, (96, 96, 96), org, sp, 0.0, probe=4)
    assert_same_mesh(dense, mesh.marching_cubes_sparse(sv, 0.0, want_keys=True))
    ref = S.select(host(vol), 0.0, probe=4)
    np.testing.assert_array_equal(host(sv.coords), ref["coords"])
    assert sv.rounds == ref["rounds"] and sv.evaluations == ref["evaluations"] and sv.probe == 4
    print(f"{which} 96^3: {sv.n_bricks} bricks, {sv.rounds} rounds, evaluated share {sv.evaluations / 96 ** 3:.3f}")


def test_selection_256_evaluates_a_quarter_at_most():
    from customnerf_amd import mesh
    vol, org, sp, dense = analytic("sphere", 256)
    sv = mesh.sparse_volume(sphere_fn, (256, 256, 256), org, sp, 0.0, probe=4)
    assert_same_mesh(dense, mesh.marching_cubes_sparse(sv, 0.0, want_keys=True))
    print(f"sphere 256^3: {sv.n_bricks} bricks, {sv.rounds} rounds, evaluated share {sv.evaluations / 256 ** 3:.3f}")
    assert sv.evaluations <= 0.25 * 256 ** 3                                     # the restatement of the rule alone gives 0.177


def test_selection_probe_1_finds_every_speckle():
    from customnerf_amd import mesh
    name, vol, level, sp, org = VOLUMES[2]
    g = torch.from_numpy(vol).cuda()
    hi = torch.tensor(vol.shape, device="cuda") - 1
    o, s = torch.tensor(org, dtype=torch.float32, device="cuda"), torch.tensor(sp, dtype=torch.float32, device="cuda")

    def fn(x):                                                                  # the stored value of the lattice point x was made from
        i = torch.minimum(torch.round((x - o) / s).long().clamp(min=0), hi)
        return g[i[:, 0], i[:, 1], i[:, 2]]
    sv = mesh.sparse_volume(fn, vol.shape, org, sp, level, probe=1)
    assert_same_mesh(mesh.marching_cubes(g, level, spacing=sp, origin=org), mesh.marching_cubes_sparse(sv, level, want_keys=True))


# ------------------------------------------------------------------------------------------------ 4. open and converged
def test_missing_neighbour_is_refused():
    from customnerf_amd import mesh
    name, vol, level, sp, org = VOLUMES[0]
    sv = mesh.sparse_volume_from_dense(torch.from_numpy(vol).cuda(), level, spacing=sp, origin=org)
    coords, values = host(sv.coords), host(sv.values)
    crossing = np.flatnonzero(S.state(values, coords, host(sv.nbr), vol.shape, level) & 1)
    keep = np.arange(len(coords)) != crossing[len(crossing) // 2]
    coords, values = coords[keep], values[keep]
    cut = mesh.SparseVolume(vol.shape, org, sp, torch.from_numpy(coords).cuda(), torch.from_numpy(values).cuda(),
                            torch.from_numpy(S.build_nbr(coords, vol.shape)).cuda())
    n_open = S.marching_cubes(values, coords, S.build_nbr(coords, vol.shape), vol.shape, level)["open"]
    assert n_open > 0
    with pytest.raises(ValueError, match=f"{n_open} open bricks"):
        mesh.marching_cubes_sparse(cut, level)


def test_max_rounds_runs_out():
    from customnerf_amd import mesh
    vol, org, sp, dense = analytic("sphere", 96)
    with pytest.raises(ValueError, match="max_rounds"):
        mesh.sparse_volume(sphere_fn, (96, 96, 96), org, sp, 0.0, probe=4, max_rounds=1)
    assert mesh.sparse_volume(sphere_fn, (96, 96, 96), org, sp, 0.0, probe=4, max_rounds=2).rounds == 2


def test_empty_field():
    from customnerf_amd import mesh
    sv = mesh.sparse_volume(lambda x: torch.full((len(x),), -1.0, device=x.device), (40, 33, 21), (0, 0, 0), (1, 1, 1), 0.0)
    assert sv.n_bricks == 0 and sv.rounds == 0 and sv.nbr.shape == (0, 27)
    v, f, n, keys = mesh.marching_cubes_sparse(sv, 0.0, want_keys=True)
    torch.cuda.synchronize()
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3) and keys.shape == (0,)
    sv = mesh.sparse_volume_from_dense(torch.full((9, 9, 9), -1.0, device="cuda"), 0.0)
    assert sv.n_bricks == 0 and mesh.marching_cubes_sparse(sv, 0.0)[1].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ 5. through the renderer
def mesh_keys(m, R):
    """extract_mesh returns no keys, so a mesh dict is put in an order of its own that both paths share: the vertices, as the bits of
    (position, normal), sorted; the faces renumbered into that order and sorted by row"""
    v, n, f = host(m['verts']), host(m['normals']), host(m['faces'])
    rec = np.concatenate([BITS(v), BITS(n)], 1)
    order = np.lexsort(rec.T[::-1])
    inv = np.empty(len(order), dtype=np.int64)
    inv[order] = np.arange(len(order))
    return rec[order], S.sorted_rows(inv[f.astype(np.int64)])


def assert_same_extraction(dense, sparse, R):
    assert sparse['volume'] is None and dense['volume'] is not None and len(dense['faces']) > 500
    dv, df = mesh_keys(dense, R)
    sv, sf = mesh_keys(sparse, R)
    assert len(np.unique(dv, axis=0)) == len(dv)                                 # (position, normal) names a vertex: the order is defined
    np.testing.assert_array_equal(sv, dv)
    np.testing.assert_array_equal(sf, df)
    info = sparse['sparse']
    assert set(info) == {'bricks', 'evaluations', 'rounds', 'points'} and info['points'] == R ** 3
    assert 0 < info['bricks'] * 512 < info['evaluations'] < R ** 3
    assert set(sparse) == set(dense) | {'sparse'}


def assert_density_ignores_batching(model):
    """density() of one point set in two batch compositions: identical bits (the dense path relies on it across `chunk` already)"""
    x = (torch.rand(5000, 3, device="cuda") - 0.5).contiguous()
    whole = model.density(x)['sigma'].reshape(-1).float()
    perm = torch.randperm(5000, device="cuda")
    parts = torch.cat([model.density(x[perm[:1237]].contiguous())['sigma'].reshape(-1).float(),
                       model.density(torch.cat([x[perm[1237:]], x[:300] * 0.5]).contiguous())['sigma'].reshape(-1).float()[:5000 - 1237]])
    assert torch.equal(whole[perm].view(torch.int32), parts.view(torch.int32))


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_extract_mesh_sparse_equals_dense(dtype_guard, fp16):
    model = gaussian_model(dtype_guard, fp16)
    with torch.no_grad():
        assert_density_ignores_batching(model)
    dense = model.extract_mesh(resolution=96, threshold=10.0, aabb=AABB)
    assert 'sparse' not in dense and set(dense) == {'verts', 'faces', 'normals', 'colors', 'volume', 'threshold', 'uvs', 'texture',
                                                     'texture_layout'}
    assert_same_extraction(dense, model.extract_mesh(resolution=96, threshold=10.0, aabb=AABB, sparse=True), 96)
    with pytest.raises(ValueError):
        model.extract_mesh(resolution=96, threshold=10.0, aabb=AABB, sparse=True, sparse_probe=0)


def test_extract_mesh_sparse_part_fg(dtype_guard):
    model = gaussian_model(dtype_guard, False)
    model.opt.soft_mask = True
    kw = dict(resolution=96, threshold=2.0, aabb=AABB, part='fg')
    assert_same_extraction(model.extract_mesh(**kw), model.extract_mesh(sparse=True, **kw), 96)


def test_extract_mesh_sparse_feeds_the_later_stages(dtype_guard, tmp_path):
    import glb_testlib
    model = gaussian_model(dtype_guard, True)
    kw = dict(resolution=96, threshold=10.0, aabb=AABB, keep_largest=True, target_faces=2000, texture=64, texture_layout='projected',
              bake_from='source', deviation=True)
    dense, sparse = model.extract_mesh(**kw), model.extract_mesh(sparse=True, **kw)
    assert set(sparse) == set(dense) | {'sparse'} and sparse['volume'] is None
    assert sparse['faces'].shape == dense['faces'].shape and sparse['texture'].shape == (64, 64, 3)
    assert sparse['deviation']['hausdorff'] < 2.0 / 95
    p = str(tmp_path / "x.glb")
    m = model.save_mesh(p, resolution=96, threshold=10.0, aabb=AABB, sparse=True, sparse_probe=2)
    doc, blob = glb_testlib.parse_glb(p)
    prim = doc["meshes"][0]["primitives"][0]
    pos = glb_testlib.read_accessor(doc, blob, prim["attributes"]["POSITION"])
    assert 'sparse' in m and m['sparse']['rounds'] >= 2 and len(pos) == len(m['verts'])
    np.testing.assert_array_equal(BITS(pos.astype(np.float32)), BITS(host(m['verts'])))


# ------------------------------------------------------------------------------------------------ 6. reproducibility
def test_two_runs_give_the_same_bytes():
    from customnerf_amd import mesh
    vol, org, sp, dense = analytic("sphere", 96)
    runs = []
    for _ in range(2):
        sv = mesh.sparse_volume(sphere_fn, (96, 96, 96), org, sp, 0.0, probe=4)
        runs.append([host(t).tobytes() for t in mesh.marching_cubes_sparse(sv, 0.0, want_keys=True)] + [host(sv.coords).tobytes(),
                                                                                                          host(sv.values).tobytes()])
    assert runs[0] == runs[1]
