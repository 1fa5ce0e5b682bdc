"""CPU: what the winding-number feature promises without a GPU — the four entry points are bound and exported and decide their return codes
before any launch, the Python layer validates, the new defaults are what the documents say — and three conditions on the REFERENCE
alone (tests/winding_restatement.py exact(), over the fixtures and queries of tests/winding_testlib.py) that keep the GPU tests of
tests/test_gpu_mesh_winding.py honest:
  (a) on a closed fixture the exact w is an integer (to 1e-9) for every query at least 1e-6 diagonals off the surface;
  (b) the restated walk at beta = 2, in float64, is within 0.25 of the exact w on every fixture: the far field cannot flip `contains`
      outside the band |w - 0.5| <= 0.25;
  (c) on the open fixtures at most 1 % of the queries lie in that band, so `contains` is asked of nearly all of them.
Measured (printed by the tests): (a) <= 2.9e-15; (b) <= 0.0336 (nested), 0.0259 (torus), <= 0.02 elsewhere; (c) 0.37 % (holed_sphere),
0.49 % (soup)."""
import ctypes as C
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import winding_restatement as W  # noqa: E402
import winding_testlib as L  # noqa: E402

NAMES4 = ("cnerf_mesh_winding_workspace_bytes", "cnerf_mesh_winding_build", "cnerf_mesh_winding_query", "cnerf_mesh_bvh_signed_distance")


def test_abi_names_and_version():
    from customnerf_amd import _lib
    assert _lib.lib.cnerf_abi_version() == 8
    header = open(os.path.join(HERE, "..", "include", "customnerf_hip.h")).read()
    for name in NAMES4:
        assert name in _lib.SIGNATURES and callable(getattr(_lib.lib, name)) and f"int {name}(" in header
    assert "#define CNERF_ABI_VERSION 8" in header


def test_return_codes_before_any_launch():
    from customnerf_amd import _lib
    lib = _lib.lib
    need, mneed = C.c_uint64(0), C.c_uint64(0)
    assert lib.cnerf_mesh_bvh_workspace_bytes(1000, 2000, C.byref(need)) == 0
    assert lib.cnerf_mesh_winding_workspace_bytes(1000, 2000, C.byref(mneed)) == 0
    assert lib.cnerf_mesh_winding_workspace_bytes(1000, 2000, None) == -2
    assert lib.cnerf_mesh_winding_workspace_bytes(1 << 31, 2000, C.byref(mneed)) == -1
    assert lib.cnerf_mesh_winding_workspace_bytes(1000, 1 << 31, C.byref(mneed)) == -1
    for F in (0, 1, 4, 5, 13, 2000, 2 ** 20 + 1):                                  # 32 bytes per heap index of a tree of depth D
        assert lib.cnerf_mesh_winding_workspace_bytes(8, F, C.byref(mneed)) == 0
        NL = max((F + 3) // 4, 1)
        D = 0 if NL <= 1 else (NL - 1).bit_length()
        assert mneed.value >= 32 * 2 ** (D + 1) and mneed.value % 16 == 0, F
    assert lib.cnerf_mesh_winding_workspace_bytes(1000, 2000, C.byref(mneed)) == 0
    one, odd, big = C.c_void_p(4096), C.c_void_p(4097), 1 << 40

    def build(ws=one, nbytes=big, V=1000, F=2000, mom=one, mbytes=big):
        return lib.cnerf_mesh_winding_build(ws, nbytes, V, F, mom, mbytes, None)

    def query(ws=one, nbytes=big, V=1000, F=2000, mom=one, mbytes=big, pts=one, Q=8, beta=2.0, w=one):
        return lib.cnerf_mesh_winding_query(ws, nbytes, V, F, mom, mbytes, pts, Q, beta, w, None, None)

    def signed(ws=one, nbytes=big, V=1000, F=2000, mom=one, mbytes=big, pts=one, Q=8, beta=2.0, sd=one, face=one, w=None):
        return lib.cnerf_mesh_bvh_signed_distance(ws, nbytes, V, F, mom, mbytes, pts, Q, beta, sd, face, w, None, None)

    assert build(ws=None) == -2 and build(mom=None) == -2
    assert build(nbytes=need.value - 1) == -1 and build(mbytes=mneed.value - 1) == -1 and build(ws=odd) == -1 and build(mom=odd) == -1
    assert build(V=1 << 31) == -1 and build(F=1 << 31) == -1
    for call in (query, signed):
        assert call(ws=None) == -2 and call(mom=None) == -2 and call(pts=None) == -2
        assert call(nbytes=need.value - 1) == -1 and call(mbytes=mneed.value - 1) == -1 and call(ws=odd) == -1 and call(mom=odd) == -1
        assert call(Q=1 << 31) == -1 and call(V=1 << 31) == -1 and call(F=1 << 31) == -1
        assert call(beta=0.999) == -1 and call(beta=float("nan")) == -1 and call(beta=-math.inf) == -1 and call(beta=0.0) == -1
        assert call(Q=0) == 0 and call(Q=0, beta=math.inf) == 0 and call(Q=0, beta=1.0) == 0 and call(Q=0, pts=None) == 0
    assert query(w=None) == -2 and signed(sd=None) == -2 and signed(face=None) == -2
    assert query(Q=0, w=None) == 0 and signed(Q=0, sd=None, face=None) == 0


def test_python_validation_and_defaults():
    from customnerf_amd import mesh
    from customnerf_amd.nerf.renderer import NeRFRenderer
    bvh = mesh.MeshBVH(None, 0, 0, 0, 0, 0)
    cpu = torch.zeros(4, 3)
    for fn in (mesh.winding_number, mesh.contains, mesh.signed_distance):
        with pytest.raises(ValueError, match=fn.__name__ if fn is not mesh.contains else "winding_number"):
            fn(object(), cpu)
        with pytest.raises(ValueError, match="beta"):
            fn(bvh, cpu, beta=0.5)
        with pytest.raises(ValueError, match="beta"):
            fn(bvh, cpu, beta=float("nan"))
        with pytest.raises(RuntimeError):
            fn(bvh, cpu)
    f = torch.zeros(1, 3, dtype=torch.int32)
    for kw in (dict(), dict(resolution=8, voxel=0.1), dict(resolution=1), dict(voxel=0.0), dict(voxel=math.inf), dict(resolution=8, beta=0.5),
               dict(resolution=8, offset=math.nan), dict(resolution=8, pad=0)):
        with pytest.raises(ValueError, match="voxel_remesh"):
            mesh.voxel_remesh(cpu, f, **kw)
    with pytest.raises(RuntimeError):
        mesh.voxel_remesh(cpu, f, resolution=8)
    sig = lambda fn: inspect.signature(fn).parameters                                # noqa: E731
    assert sig(mesh.winding_number)['beta'].default == 2.0 and sig(mesh.winding_number)['want_stats'].default is False
    assert sig(mesh.contains)['beta'].default == 2.0
    assert sig(mesh.signed_distance)['beta'].default == 2.0 and sig(mesh.signed_distance)['want_winding'].default is False
    p = sig(mesh.voxel_remesh)
    assert (p['resolution'].default, p['voxel'].default, p['offset'].default, p['beta'].default, p['probe'].default, p['pad'].default,
            p['chunk'].default) == (None, None, 0.0, 2.0, 2, 2, 2 ** 21)
    assert sig(NeRFRenderer.extract_mesh)['remesh'].default is None and "remesh" in NeRFRenderer.save_mesh.__doc__
    assert "not an optimum measured here" in " ".join(mesh.winding_number.__doc__.split())


@pytest.mark.parametrize("name", L.NAMES)
def test_reference_conditions(name):
    c = L.case(name)
    fin = np.isfinite(c['q']).all(1)
    e = c['exact']
    assert (e[~fin] == 0).all() and (c['w2'][~fin] == 0).all()
    off = c['off'] & fin
    if c['closed']:
        a = float(np.abs(e[off] - np.round(e[off])).max())
        print(f"{name}: (a) max |w - round(w)| = {a:.3g} over {int(off.sum())} queries")
        assert a <= 1e-9
    b = float(np.abs(c['w2_64'] - e)[fin].max())
    print(f"{name}: (b) max |walk64(beta = 2) - exact| = {b:.4g}")
    assert b < 0.25
    if not c['closed']:
        share = float((~c['clear'])[fin].mean())
        print(f"{name}: (c) {100 * share:.2f} % of the queries in the band")
        assert share <= 0.01
    # the fixtures are what the GPU tests take them for
    want = {"icosphere": {0, 1}, "torus": {0, 1}, "nested": {0, 1, 2}, "inward": {-1, 0}, "two_spheres": {0, 1, 2}, "bad_faces": {0, 1}, "empty": {0}}
    if name in want:
        assert set(np.round(e[off]).astype(int).tolist()) == want[name]
    assert len(c['q']) >= 1400 and (c['tri2'] + c['acc2'] <= c['triinf']).all()


def test_restated_walk_is_the_exact_sum_at_beta_inf():
    """beta = inf accepts no node: the float32 walk differs from the float64 sum by rounding alone, far inside n_terms 2^-20"""
    for name in L.NAMES:
        c = L.case(name)
        off = c['off']
        n = np.maximum(c['triinf'], 1)
        assert (np.abs(c['winf'] - c['exact'])[off] <= n[off] * 2.0 ** -20).all(), name
        assert (c['triinf'][np.isfinite(c['q']).all(1)] == c['tree']['n']).all()


def test_restated_moments_are_consistent():
    """the root's area is the mesh's, its area vector is ~0 for a closed mesh, and every node's ball holds the vertices below it"""
    for name in ("icosphere", "torus", "soup", "bad_faces"):
        c = L.case(name)
        tr, mom = c['tree'], c['mom']
        tri = tr['rec'][tr['valid']].astype(np.float64)
        area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
        assert abs(float(mom[1, 1, 3]) - area.sum()) <= 1e-5 * area.sum()
        if c['closed']:
            assert np.abs(mom[1, 1, :3]).max() <= 1e-5 * area.sum()
        D, NL = tr['D'], tr['NL']
        for d in range(D + 1):
            for j in range(1 << d):
                l0, l1 = (j * NL) >> d, ((j + 1) * NL) >> d
                pts = tr['rec'][4 * l0:4 * l1][tr['valid'][4 * l0:4 * l1]].reshape(-1, 3).astype(np.float64)
                p, r = mom[(1 << d) + j, 0, :3].astype(np.float64), float(mom[(1 << d) + j, 0, 3])
                if len(pts):
                    assert np.linalg.norm(pts - p, axis=1).max() <= r * (1 + 1e-5) + 1e-6
                else:
                    assert r == -1.0
    assert W.moments(L.case("empty")['tree']).shape == (2, 2, 4) and L.case("empty")['mom'][1, 0, 3] == -1.0
