"""CPU: the C-ABI of cnerf_mesh_topology* / cnerf_mesh_holes_* up to the point where it would launch, the argument checks of
mesh.topology, mesh.fill_holes and extract_mesh(fill_holes=, topology=), and the NumPy restatement (tests/holes_restatement.py) on meshes
whose answers are known."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import holes_restatement as H  # noqa: E402
import mesh_testlib as L  # noqa: E402
import qem_restatement as Q  # noqa: E402
from holes_testlib import holed_sphere, meshes  # noqa: E402

ROOT = os.path.dirname(HERE)
NAMES = ("cnerf_mesh_holes_workspace_bytes", "cnerf_mesh_topology", "cnerf_mesh_topology_loops", "cnerf_mesh_holes_count",
         "cnerf_mesh_holes_emit")
EINVAL, ENULL = -1, -2
FAKE = 1 << 20                                                                   # never dereferenced: every call returns before a launch
BIG = 1 << 40                                                                    # a workspace size no check finds too small


def test_abi_declared_bound_and_exported():
    from customnerf_amd import _lib
    src = open(os.path.join(ROOT, "include", "customnerf_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8
    rules = src[src.index("Topology report and hole filling"):src.index("int cnerf_mesh_holes_workspace_bytes(")]
    for word in ("pinched", "simple", "fp64 in loop order", "rounded once"):
        assert word in rules, word


def _call(name, **k):
    from customnerf_amd._lib import lib
    a = dict(verts=FAKE, normals=None, faces=FAKE, V=8, F=4, max_edges=0, ws=FAKE, ws_bytes=BIG, counts=FAKE, loops=FAKE, max_loops=4,
             vo=FAKE, no=None, fo=FAKE, max_verts=9, max_faces=8, stream=None)
    a.update(k)
    order = {"cnerf_mesh_topology": ("faces", "V", "F", "ws", "ws_bytes", "counts", "stream"),
             "cnerf_mesh_topology_loops": ("V", "F", "ws", "ws_bytes", "loops", "max_loops", "stream"),
             "cnerf_mesh_holes_count": ("faces", "V", "F", "max_edges", "ws", "ws_bytes", "counts", "stream"),
             "cnerf_mesh_holes_emit": ("verts", "normals", "V", "faces", "F", "max_edges", "ws", "ws_bytes", "vo", "no", "fo", "max_verts",
                                       "max_faces", "stream")}[name]
    return getattr(lib, name)(*[a[n] for n in order])


@pytest.mark.parametrize("name", NAMES[1:])
def test_entry_points_refuse_or_accept_before_launch(name):
    for bad in (dict(V=1 << 31), dict(F=1 << 31), dict(F=0x2AAAAAAB)):
        assert _call(name, **bad) == EINVAL, bad
    assert _call(name, ws_bytes=256) == EINVAL                                   # a workspace that is too small
    assert _call(name, ws=FAKE + 4) == EINVAL                                    # or not 16-byte aligned
    nulls = {"cnerf_mesh_topology": ("faces", "ws", "counts"), "cnerf_mesh_topology_loops": ("ws", "loops"),
             "cnerf_mesh_holes_count": ("faces", "ws", "counts"), "cnerf_mesh_holes_emit": ("verts", "faces", "ws", "vo", "fo")}[name]
    for k in nulls:
        assert _call(name, **{k: None}) == ENULL, k
        assert _call(name, V=1 << 31, **{k: None}) == EINVAL                     # the values are looked at first
        assert _call(name, F=0, **{k: None}) == 0                                # an empty mesh: accepted without a launch
    assert _call(name, F=0) == 0 and _call(name, F=0, V=0) == 0
    if "holes_" in name:
        assert _call(name, max_edges=1) == EINVAL and _call(name, max_edges=2) == EINVAL
        assert _call(name, max_edges=2, faces=None) == EINVAL
    if name.endswith("_loops"):
        assert _call(name, max_loops=0, loops=None) == 0                         # no loop asked for: nothing to launch
    if name.endswith("_emit"):
        assert _call(name, V=0, verts=None, max_verts=0, vo=None, F=0) == 0


def test_workspace_query():
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib
    n = C.c_uint64(0)
    assert lib.cnerf_mesh_holes_workspace_bytes(1 << 31, 4, C.byref(n)) == EINVAL
    assert lib.cnerf_mesh_holes_workspace_bytes(8, 0x2AAAAAAB, C.byref(n)) == EINVAL
    assert lib.cnerf_mesh_holes_workspace_bytes(8, 4, None) == ENULL
    assert mesh.holes_workspace_bytes(0, 0) >= 256 and mesh.holes_workspace_bytes(0, 0) % 256 == 0
    V, F = 100000, 200000
    assert 17 * V + 51 * F <= mesh.holes_workspace_bytes(V, F) <= 17 * V + 51 * F + 36 * (3 * F // 256 + 1) + 12 * 256


def test_python_side_rejects_before_the_device():
    import torch
    from customnerf_amd import mesh
    from customnerf_amd.nerf.renderer import NeRFRenderer
    sig = inspect.signature(NeRFRenderer.extract_mesh).parameters
    assert sig["fill_holes"].default is False and sig["topology"].default is False
    assert [p.default for p in inspect.signature(mesh.fill_holes).parameters.values()][2:] == [None, None]
    for bad in (dict(fill_holes=2), dict(fill_holes='x'), dict(fill_holes=True, simplify=4), dict(fill_holes=0), dict(fill_holes=3.0),
                dict(fill_holes=8, simplify=2)):
        with pytest.raises(ValueError):
            NeRFRenderer.extract_mesh(object(), **bad)                           # before anything of the renderer is looked at
    v, f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        mesh.topology(v, f)                                                      # no CPU path
    with pytest.raises(RuntimeError):
        mesh.fill_holes(v, f)
    for bad in (2, 0, -1, 'x', 3.5, True, 1 << 32):
        with pytest.raises(ValueError):
            mesh.fill_holes(v, f, max_edges=bad)


# ------------------------------------------------------------------------------------------------ the restatement on known meshes
#            boundary edges, loops, simple loops, pinched vertices, euler
EXPECTED = {"cut_sphere": (64, 1, 1, 0, 1), "planar_grid": (64, 1, 1, 0, 1), "two_tori": (0, 0, 0, 0, 0), "noise": (1380, 132, 132, 0, -138),
            "sphere": (0, 0, 0, 0, 2), "holed_sphere": (11, 3, 3, 0, -1), "pinched_sphere": (6, 1, 0, 1, 0)}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_restatement_topology(name):
    v, f, _ = meshes()[name]
    t = H.topology(v, f)
    be, loops, simple, pinched, euler = EXPECTED[name]
    assert (t["boundary_edges"], t["boundary_loops"], t["simple_loops"], t["pinched_vertices"], t["euler"]) == EXPECTED[name]
    assert t["nonmanifold_edges"] == 0 and t["degenerate_faces"] == 0 and t["faces"] == len(f)
    assert t["euler"] == Q.euler(f) and t["boundary_edges"] == Q.check_manifold(f)
    assert t["watertight"] == (be == 0) and int(t["loop_lengths"].sum()) == be and len(t["loop_lengths"]) == loops
    assert t["vertices_used"] == len(np.unique(f)) and t["components"] == (2 if name == "two_tori" else t["components"])
    if name in ("cut_sphere", "planar_grid"):
        assert t["loop_lengths"].tolist() == [64] and t["components"] == 1
    if name == "holed_sphere":
        assert sorted(t["loop_lengths"].tolist()) == [3, 4, 4] and t["vertices_used"] == 256 and t["components"] == 1
    if name == "pinched_sphere":
        assert t["loop_lengths"].tolist() == [6]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_restatement_fill(name):
    v, f, n = meshes()[name]
    before = H.topology(v, f)
    vo, fo, no, info = H.fill_holes(v, f, n)
    assert vo.dtype == np.float32 and fo.dtype == np.int32 and (no is None) == (n is None)
    assert np.array_equal(vo[:len(v)].view(np.uint32), v.view(np.uint32)) and np.array_equal(fo[:len(f)], f)      # the prefix
    assert n is None or np.array_equal(no[:len(v)].view(np.uint32), n.view(np.uint32))
    assert info["filled"] == before["simple_loops"] and info["skipped_long"] == 0
    assert info["skipped_pinched"] == before["boundary_loops"] - before["simple_loops"]
    assert len(vo) == len(v) + info["new_vertices"] and len(fo) == len(f) + info["new_faces"]
    after = H.topology(vo, fo)
    assert after["euler"] == before["euler"] + info["filled"] and after["nonmanifold_edges"] == 0 and after["degenerate_faces"] == 0
    if before["simple_loops"] == before["boundary_loops"]:
        assert Q.check_manifold(fo) == 0 and after["watertight"]
    else:
        assert np.array_equal(fo, f) and np.array_equal(vo, v)                   # the pinched mesh: nothing to fill
    assert after["euler"] == {"noise": -6, "holed_sphere": 2}.get(name, after["euler"])
    if no is not None and info["new_vertices"]:
        new = no[len(v):].astype(np.float64)
        assert np.allclose(np.linalg.norm(new, axis=1), 1.0, atol=1e-6)
    if name in ("cut_sphere", "planar_grid"):
        assert info == {"filled": 1, "skipped_pinched": 0, "skipped_long": 0, "new_vertices": 1, "new_faces": 64}
        assert H.fill_holes(v, f, n, max_edges=63)[3] == {"filled": 0, "skipped_pinched": 0, "skipped_long": 1, "new_vertices": 0, "new_faces": 0}
        assert H.fill_holes(v, f, n, max_edges=64)[3] == info
    if name == "cut_sphere":                                                     # the cap's normal points out of the cut: down
        assert no[len(v), 2] < -0.99 and abs(float(vo[len(v), 2]) + 1.0) < 1e-6


def test_restatement_three_loop_restores_the_removed_face():
    v, f, removed = holed_sphere()
    vo, fo, _, info = H.fill_holes(v, f)
    assert info == {"filled": 3, "skipped_pinched": 0, "skipped_long": 0, "new_vertices": 2, "new_faces": 9}
    tri = [t for t in fo[len(f):].tolist() if max(t) < len(v)]
    assert len(tri) == 1 and tuple(tri[0]) in {tuple(np.roll(removed, s)) for s in range(3)}
    only3 = H.fill_holes(v, f, max_edges=3)
    assert only3[3] == {"filled": 1, "skipped_pinched": 0, "skipped_long": 2, "new_vertices": 0, "new_faces": 1} and len(only3[0]) == len(v)


def test_restatement_refuses_bad_meshes():
    v, f = L.octahedron_sphere(1)
    fan = np.concatenate([f, [[f[0, 0], f[0, 1], len(v)]]]).astype(np.int32)     # a third face on the edge (f00, f01)
    v3 = np.concatenate([v, [[2.0, 2.0, 2.0]]]).astype(np.float32)
    t = H.topology(v3, fan)
    assert t["nonmanifold_edges"] == 1 and not t["watertight"] and t["boundary_edges"] == 2 and t["simple_loops"] == 0
    with pytest.raises(ValueError):
        H.fill_holes(v3, fan)
    rep = f.copy()
    rep[3, 2] = rep[3, 0]
    assert H.topology(v, rep)["degenerate_faces"] == 1
    with pytest.raises(ValueError):
        H.fill_holes(v, rep)
    flip = f.copy()
    flip[5] = flip[5, ::-1]                                                      # one face wound the other way
    assert H.topology(v, flip)["nonmanifold_edges"] == 3
    with pytest.raises(ValueError):
        H.fill_holes(v, flip)
    out = f.copy()
    out[2, 1] = len(v)
    for fn in (H.topology, H.fill_holes):
        with pytest.raises(ValueError):
            fn(v, out)
