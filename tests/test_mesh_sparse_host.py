"""CPU: the C-ABI of cnerf_marching_cubes_sparse_* up to the point where it would launch, and the NumPy restatement of brick-sparse
extraction (tests/mc_sparse_restatement.py) pinned to the restatement of the dense pass."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mc_restatement as R  # noqa: E402
import mc_sparse_restatement as S  # noqa: E402

ROOT = os.path.dirname(HERE)
NAMES = ("cnerf_marching_cubes_sparse_workspace_bytes", "cnerf_marching_cubes_sparse_count", "cnerf_marching_cubes_sparse_emit")


def test_abi_declared_bound_and_exported():
    from customnerf_amd import _lib
    src = open(os.path.join(ROOT, "include", "customnerf_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8


def test_workspace_bytes():
    from customnerf_amd import mesh
    for n in (1, 7, 5268):
        b = mesh.sparse_workspace_bytes(n)
        assert 6 * 512 * n <= b <= 6.1 * 512 * n + 7 * 256                       # the dense regions over n * 512 points + 2 bytes a brick
    assert mesh.sparse_workspace_bytes(0) == 256 and mesh.BRICK == 8


def test_argument_checks_reject_before_launch():
    from customnerf_amd._lib import lib
    EINVAL, ENULL = -1, -2
    out = C.c_uint64(0)
    size = lib.cnerf_marching_cubes_sparse_workspace_bytes
    assert size(1 << 22, C.byref(out)) == EINVAL and size(4, None) == ENULL
    assert size(4, C.byref(out)) == 0 and out.value > 0
    wsb = out.value
    fake = 1 << 20                                   # never dereferenced: every call below returns before a launch
    count = lambda **k: lib.cnerf_marching_cubes_sparse_count(*[{**dict(values=fake, coords=fake, nbr=fake, n=4, nx=16, ny=16, nz=16, level=0.0, ws=fake,  # noqa: E731
                                                                    wsb=wsb, state=None, counts=fake, stream=None), **k}[a] for a in
                                                                ("values", "coords", "nbr", "n", "nx", "ny", "nz", "level", "ws", "wsb", "state", "counts", "stream")])
    assert count(n=0) == 0 and count(n=0, values=None, ws=None, counts=None) == 0            # nothing to do: no launch
    for k in ("values", "coords", "nbr", "ws", "counts"):
        assert count(**{k: None}) == ENULL, k
    assert count(values=None, nx=1) == ENULL                                                  # NULLs are reported first
    for k in ("nx", "ny", "nz"):
        assert count(**{k: 1}) == EINVAL and count(**{k: (1 << 20) + 1}) == EINVAL, k
    assert count(nx=1 << 20, ny=2, nz=2, wsb=wsb - 1) == EINVAL
    assert count(n=1 << 22, wsb=1 << 40) == EINVAL
    assert count(wsb=wsb - 1) == EINVAL and count(ws=fake + 4) == EINVAL                       # short / misaligned workspace
    f3, s3 = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    emit = lambda **k: lib.cnerf_marching_cubes_sparse_emit(*[{**dict(values=fake, coords=fake, nbr=fake, n=4, nx=16, ny=16, nz=16, level=0.0, org=f3,  # noqa: E731
                                                                  sp=s3, ws=fake, wsb=wsb, verts=fake, normals=None, faces=fake, keys=None, mv=1, mf=1,
                                                                  stream=None), **k}[a] for a in
                                                              ("values", "coords", "nbr", "n", "nx", "ny", "nz", "level", "org", "sp", "ws", "wsb", "verts",
                                                               "normals", "faces", "keys", "mv", "mf", "stream")])
    assert emit(n=0) == 0
    for k in ("values", "coords", "nbr", "org", "sp", "ws", "verts", "faces"):
        assert emit(**{k: None}) == ENULL, k
    assert emit(nz=1) == EINVAL and emit(ny=(1 << 20) + 1) == EINVAL and emit(n=1 << 22, wsb=1 << 40) == EINVAL
    assert emit(wsb=wsb - 1) == EINVAL and emit(ws=fake + 8) == EINVAL


VOLUMES = S.volumes()


@pytest.mark.parametrize("name, vol, level, sp, org", VOLUMES, ids=[v[0] for v in VOLUMES])
def test_restatement_equals_dense_restatement(name, vol, level, sp, org):
    sel = S.select(vol, level, probe=1)
    got = S.marching_cubes(sel["values"], sel["coords"], sel["nbr"], vol.shape, level, sp, org)
    assert got["open"] == 0
    assert (np.diff([(int(c[0]) * 10 ** 6 + int(c[1])) * 10 ** 6 + int(c[2]) for c in sel["coords"]]) > 0).all()   # unique, sorted
    assert (sel["nbr"][:, 13] == np.arange(len(sel["coords"]))).all()
    v, f, n = R.marching_cubes(vol, level, sp, org)
    assert len(f) > 0 and len(np.unique(got["keys"])) == len(got["keys"]) == len(v)
    gv, gf, gn = S.reorder(got["verts"], got["faces"], got["normals"], got["keys"])
    assert np.array_equal(gv.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(gn.view(np.uint32), n.view(np.uint32))
    assert np.array_equal(gf, S.sorted_rows(f))
    # keys are the dense pass's (point, axis) numbering: sorted, they are what it counts through
    assert S.marching_cubes(sel["values"], sel["coords"], sel["nbr"], vol.shape, level, sp, org, normals=False)["normals"] is None


def test_probe_selection_matches_every_point_selection():
    """probe = 4 sees the speckled sphere's main surface; what it finds is a subset of probe = 1, and the sphere alone (no speckle
    smaller than the probe) gives the identical list."""
    import mesh_testlib
    sphere, vol, sp, org = mesh_testlib.speckled_sphere(56)
    full, coarse = S.select(sphere, 0.0, probe=1), S.select(sphere, 0.0, probe=4)
    assert np.array_equal(full["coords"], coarse["coords"]) and coarse["evaluations"] < full["evaluations"]
    a = {tuple(c) for c in S.select(vol, 0.0, probe=4)["coords"].tolist()}
    b = {tuple(c) for c in S.select(vol, 0.0, probe=1)["coords"].tolist()}
    assert a <= b


def test_deleted_brick_is_reported_open():
    name, vol, level, sp, org = VOLUMES[0]
    sel = S.select(vol, level, probe=1)
    st = S.state(sel["values"], sel["coords"], sel["nbr"], vol.shape, level)
    assert ((st & 1) <= (st >> 1)).all()                                        # converged: every crossing brick is complete
    victim = int(np.flatnonzero(st & 1)[len(np.flatnonzero(st & 1)) // 2])      # a crossing brick: its crossing neighbours lose one
    keep = np.arange(len(sel["coords"])) != victim
    coords, values = sel["coords"][keep], sel["values"][keep]
    got = S.marching_cubes(values, coords, S.build_nbr(coords, vol.shape), vol.shape, level, sp, org)
    assert got["open"] > 0


def test_empty_field_selects_nothing():
    vol = np.full((12, 9, 10), -1.0, dtype=np.float32)
    sel = S.select(vol, 0.0, probe=4)
    assert len(sel["coords"]) == 0 and sel["rounds"] == 0


def test_python_side_rejects_before_the_device():
    import torch
    from customnerf_amd import mesh
    from customnerf_amd.nerf.renderer import NeRFRenderer
    import inspect
    sig = inspect.signature(NeRFRenderer.extract_mesh).parameters
    assert sig["sparse"].default is False and sig["sparse_probe"].default == 4
    with pytest.raises(ValueError):
        mesh.sparse_volume(lambda x: x[:, 0], (8, 8, 8), (0, 0, 0), (1, 1, 1), 0.0, probe=0)
    with pytest.raises(ValueError):
        mesh.sparse_volume(lambda x: x[:, 0], (8, 1, 8), (0, 0, 0), (1, 1, 1), 0.0)
    with pytest.raises(RuntimeError):
        mesh.sparse_volume_from_dense(torch.zeros(4, 4, 4), 0.0)                # no CPU path
