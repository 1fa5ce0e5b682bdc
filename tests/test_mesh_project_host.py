"""CPU: the projection rule of csrc/mesh_bvh.hip (cnerf_mesh_bvh_project) as tests/project_restatement.py restates it, pinned on facts that
need no GPU — the sphere, thin-slab, rim and opposed-normal cases that tests/test_gpu_mesh_project.py then demands of the device bit for
bit — the argument checks of the C entry point that return before any launch, and write_obj's normal map."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import atlas_restatement as A  # noqa: E402
import project_restatement as P  # noqa: E402
import project_testlib as L  # noqa: E402
from mesh_testlib import grid  # noqa: E402

F32 = np.float32


def test_sphere_kinds_and_radii():
    """the 3240 texels of the 80-face icosphere against the 1280-face one.  The low mesh lies inside the source (its texels at radii from
    0.934 up to 1), so with reach 0.25 every texel finds the source, 2920 along the normal and 320 against it (next to the low mesh's
    vertices, which lie on the unit sphere and so outside the source's flat faces); every projected point lies between the source's inradius
    and 1.  With reach 0.02 most texels find nothing and keep their point bit for bit."""
    s = L.sphere()
    assert 0.9954 < s['inradius'] < 0.9956
    r = L.sphere_want(0.25)
    assert P.kinds(r['kind']).tolist() == [0, 2920, 320, 0]
    rad = np.linalg.norm(r['point'].astype(np.float64), axis=1)
    # a float32 point of a face: three roundings of values below 1 — within 1e-6 of the exact face, which lies in [inradius, 1]
    assert rad.min() >= s['inradius'] - 1e-6 and rad.max() <= 1.0 + 1e-6
    assert np.linalg.norm(s['x'].astype(np.float64), axis=1).min() < 0.935         # what the projection moves
    assert (r['face'] >= 0).all() and (np.abs(np.linalg.norm(r['normal'].astype(np.float64), axis=1) - 1) < 1e-6).all()
    # the offset is the distance moved along n (unit here): point = x + offset n
    np.testing.assert_allclose(s['x'] + r['offset'][:, None] * s['n'], r['point'], atol=2e-6)
    assert (r['offset'][r['kind'] == 1] >= 0).all() and (r['offset'][r['kind'] == 2] < 0).all()
    r = L.sphere_want(0.02)
    assert P.kinds(r['kind']).tolist() == [2340, 740, 160, 0]
    none = r['kind'] == 0
    np.testing.assert_array_equal(r['point'][none].view(np.uint32), s['x'][none].view(np.uint32))
    assert (r['face'][none] == -1).all() and (r['offset'][none] == 0).all() and (np.abs(r['offset']) <= F32(0.02)).all()
    # without source normals: the faces' own
    g = L.sphere_want(0.25, False)
    assert P.kinds(g['kind']).tolist() == [0, 2920, 320, 0]
    np.testing.assert_array_equal(g['face'], L.sphere_want(0.25)['face'])
    a, b, c = (s['sv'][s['sf'][g['face'], k]].astype(np.float64) for k in range(3))
    fn = np.cross(b - a, c - a)
    assert np.abs(g['normal'] - fn / np.linalg.norm(fn, axis=1, keepdims=True)).max() < 1e-6


def test_thin_slab_keeps_to_its_own_wall():
    """above, inside and just over the bottom of a wall 0.05 thick, looking up: always the top sheet (faces 0 .. 31), never the bottom
    one 0.01 away, whose faces look the other way"""
    v, f = L.slab()
    for z, off, kind in L.SLAB_HEIGHTS:
        x, n = L.slab_queries(z)
        r = P.project(v, f, None, x, n, L.SLAB_REACH)
        assert (r['kind'] == kind).all() and (r['face'] < 32).all() and (r['face'] >= 0).all(), z
        assert np.abs(r['offset'] - off).max() < 1e-6 and np.abs(r['point'][:, 2] - 0.05).max() < 1e-6
        assert (r['normal'] == np.array([0, 0, 1], F32)).all()
    # the bottom sheet answers those who look down from below it
    x, n = L.slab_queries(-0.02)
    r = P.project(v, f, None, x, -n, L.SLAB_REACH)
    assert (r['kind'] == 2).all() and (r['face'] >= 32).all() and (r['normal'] == np.array([0, 0, -1], F32)).all()


def test_rim_falls_back_to_the_closest_point():
    v, f = grid(4)
    r = P.project(v, f, None, L.RIM_X, L.RIM_N, 0.2)
    assert r['kind'][0] == 3 and r['face'][0] == 3 and r['point'][0].tolist() == [0.0, 2.0, 0.0]
    assert abs(r['offset'][0] + 0.05) < 1e-7 and r['normal'][0].tolist() == [0.0, 0.0, 1.0]
    r = P.project(v, f, None, L.RIM_X, L.RIM_N, 0.1)                               # dist2 = 0.0125 > 0.01
    assert r['kind'][0] == 0 and r['face'][0] == -1 and r['offset'][0] == 0
    np.testing.assert_array_equal(r['point'].view(np.uint32), L.RIM_X.view(np.uint32))
    # an unnormalised direction scales the offset, not the reach: |n| = 4 gives a quarter of the offset and a reach of 0.05 * 4
    r = P.project(v, f, None, L.RIM_X, 4 * L.RIM_N, 0.05)
    assert r['kind'][0] == 3 and abs(r['offset'][0] + 0.0125) < 1e-7
    assert P.project(v, f, None, L.RIM_X, 4 * L.RIM_N, 0.025)['kind'][0] == 0


def test_opposed_normals_and_degenerate_queries():
    v, f, nrm, x, n = L.opposed()
    r = P.project(v, f, nrm, x, n, 1.0)
    assert r['kind'].tolist() == [2, 2, 2] and r['face'].tolist() == [0, 1, 2] and (r['offset'] == F32(-0.25)).all()
    np.testing.assert_array_equal(r['point'], x - F32(0.25) * n)
    np.testing.assert_array_equal(r['normal'][0], np.array([3, 0, 4], F32) / F32(5))       # interpolated
    np.testing.assert_array_equal(r['normal'][1:], np.array([[1, 0, 0], [1, 0, 0]], F32))  # cancelled / not finite: the face's
    # nothing found: the query's own direction, normalised; a direction that cannot be: +z
    r = P.project(v, f, nrm, x + np.array([9, 0, 0], F32), n, 1.0)
    assert (r['kind'] == 0).all() and np.abs(r['normal'] - n / np.sqrt(F32(5))).max() < 1e-7
    bad_x = np.array([[np.nan, 0.25, 0.75], [0.5, np.inf, 0.75], [0.5, 0.25, 0.75], [0.5, 0.25, 0.75], [0.5, 0.25, 0.75], [0.5, 0.25, 0.75]], F32)
    bad_n = np.array([[2, 0, 1], [2, 0, 1], [0, 0, 0], [np.nan, 0, 1], [2, -np.inf, 1], [2, 0, 1]], F32)
    r = P.project(v, f, nrm, bad_x, bad_n, np.array([1, 1, 1, 1, 1, -1], F32))
    assert (r['kind'] == 0).all() and (r['face'] == -1).all()
    np.testing.assert_array_equal(r['point'].view(np.uint32), bad_x.view(np.uint32))
    assert r['normal'][2:5].tolist() == [[0, 0, 1]] * 3
    assert P.project(v, f, nrm, bad_x[5:], bad_n[5:], np.array([np.nan], F32))['kind'][0] == 0


def test_abi_argument_checks():
    """cnerf_mesh_bvh_project: NULL and out-of-range arguments return before any launch (no GPU work is issued here)"""
    from customnerf_amd import _lib
    lib = _lib.lib
    need = C.c_uint64(0)
    assert lib.cnerf_mesh_bvh_workspace_bytes(1000, 2000, C.byref(need)) == 0
    one, odd, big = C.c_void_p(4096), C.c_void_p(4097), 1 << 40
    pj = lib.cnerf_mesh_bvh_project

    def call(ws=one, nbytes=big, V=1000, F=2000, faces=one, normals=one, x=one, n=one, Q=8, reach=0.5, per=None):
        return pj(ws, nbytes, V, F, faces, normals, x, n, Q, reach, per, one, one, one, one, one, None, None)
    assert call(ws=None) == -2 and call(x=None) == -2 and call(n=None) == -2 and call(faces=None) == -2
    assert call(nbytes=need.value - 1) == -1 and call(ws=odd) == -1
    assert call(Q=1 << 31) == -1 and call(F=1 << 31) == -1 and call(V=1 << 31) == -1
    assert call(reach=-1.0) == -1 and call(reach=float("nan")) == -1
    # no query: no launch, whatever else is missing; every output may be NULL
    assert pj(one, big, 1000, 2000, None, None, None, None, 0, 0.5, None, None, None, None, None, None, None, None) == 0
    assert call(Q=0, reach=0.0) == 0
    from customnerf_amd import mesh
    for name in ("bake_source", "project_to_surface", "BakeSource"):
        assert callable(getattr(mesh, name))


def test_write_obj_normal_map(tmp_path):
    """with a normal map: <stem>_normal.png and the material's `norm` line; without: the bytes written before there was one"""
    from customnerf_amd import mesh
    v, f = grid(2)
    F = len(f)
    uv = A.uvs(F, 32)
    rng = np.random.default_rng(3)
    tex, nmap = (rng.integers(0, 256, (32, 32, 3)).astype(np.uint8) for _ in range(2))
    nrm = np.tile(np.array([[0, 0, 1]], F32), (len(v), 1))
    old = tmp_path / "old"
    new = tmp_path / "new"
    old.mkdir()
    new.mkdir()
    mesh.write_obj(str(old / "m.obj"), v, f, uvs=uv, normals=nrm, texture=tex)
    mesh.write_obj(str(new / "m.obj"), v, f, uvs=uv, normals=nrm, texture=tex, normal_map=nmap)
    assert sorted(os.listdir(old)) == ["m.mtl", "m.obj", "m.png"] and sorted(os.listdir(new)) == ["m.mtl", "m.obj", "m.png", "m_normal.png"]
    for name in ("m.obj", "m.png"):
        assert (old / name).read_bytes() == (new / name).read_bytes()
    mtl = (new / "m.mtl").read_text()
    assert mtl == (old / "m.mtl").read_text() + "norm m_normal.png\n"
    # the files of a call without a normal map, byte for byte as the writer made them before it knew of one
    assert (old / "m.mtl").read_text() == "newmtl material0\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd m.png\n"
    assert (old / "m.obj").read_text().startswith("# customnerf_amd mesh export\n# 9 vertices, 8 faces\nmtllib m.mtl\nv 0 0 0\n")
    np.testing.assert_array_equal(A.read_png(str(new / "m_normal.png")), nmap)
    np.testing.assert_array_equal(A.read_png(str(new / "m.png")), tex)
    plain = tmp_path / "plain"
    plain.mkdir()
    mesh.write_obj(str(plain / "p.obj"), v, f)
    assert os.listdir(plain) == ["p.obj"] and "mtllib" not in (plain / "p.obj").read_text()
    # a normal map alone still gets its material; without uvs it is refused
    mesh.write_obj(str(plain / "n.obj"), v, f, uvs=uv, normal_map=nmap)
    assert (plain / "n.mtl").read_text().endswith("illum 1\nnorm n_normal.png\n") and "map_Kd" not in (plain / "n.mtl").read_text()
    with pytest.raises(ValueError):
        mesh.write_obj(str(plain / "q.obj"), v, f, normal_map=nmap)
