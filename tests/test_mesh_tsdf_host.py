"""CPU: the C-ABI of cnerf_tsdf_* up to the point where it would launch, the argument checks of mesh.TSDFVolume and of
extract_mesh(tsdf=...), and the NumPy restatement of the fusion (tests/tsdf_restatement.py) on an analytic sphere."""
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
import tsdf_restatement as T  # noqa: E402

ROOT = os.path.dirname(HERE)
NAMES = ("cnerf_tsdf_integrate", "cnerf_tsdf_finalize", "cnerf_tsdf_face_keep")
EINVAL, ENULL = -1, -2
FAKE = 1 << 20                                                                   # never dereferenced: every call returns before a launch


def test_abi_declared_bound_and_exported():
    from customnerf_amd import _lib
    src = open(os.path.join(ROOT, "include", "customnerf_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8
    assert "DIVISIONS AND SQUARE ROOTS ARE CORRECTLY ROUNDED" in src[src.index("TSDF fusion:"):src.index("int cnerf_tsdf_integrate(")].upper()


def _integrate(**k):
    from customnerf_amd._lib import lib
    org, sp = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    cam = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    a = dict(state=FAKE, nx=8, ny=8, nz=8, org=org, sp=sp, trunc=1.0, depth=FAKE, pw=None, n=1, H=4, W=4, c2w=cam, fx=1.0, fy=1.0, cx=2.0,
             cy=2.0, conv=0, near=0.01, kind=1, stream=None)
    a.update(k)
    return lib.cnerf_tsdf_integrate(*[a[n] for n in ("state", "nx", "ny", "nz", "org", "sp", "trunc", "depth", "pw", "n", "H", "W", "c2w", "fx",
                                                      "fy", "cx", "cy", "conv", "near", "kind", "stream")])


@pytest.mark.parametrize("over", [dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=float("inf")), dict(trunc=float("nan")), dict(fx=0.0),
                                  dict(fy=0.0), dict(fx=float("inf")), dict(fy=float("nan")), dict(cx=float("inf")), dict(cy=float("nan")),
                                  dict(near=float("inf")), dict(conv=2), dict(conv=-1), dict(kind=2), dict(kind=-1),
                                  dict(nx=2048, ny=2048, nz=1024), dict(nx=1 << 20, ny=1 << 20, nz=1 << 20), dict(H=1 << 16, W=1 << 15),
                                  dict(nx=1), dict(ny=1), dict(nz=0)], ids=str)
def test_integrate_refuses_before_launch(over):
    assert _integrate(**over) == EINVAL
    assert _integrate(n=0, **over) == EINVAL                                     # also with nothing to do


def test_integrate_null_and_empty():
    for k in ("state", "depth", "c2w", "org", "sp"):
        assert _integrate(**{k: None}) == ENULL, k
    assert _integrate(n=0) == 0 and _integrate(n=0, state=None, depth=None, c2w=None) == 0        # zero views: no launch
    assert _integrate(state=None, trunc=0.0) == EINVAL                           # the values are looked at first


def test_finalize_and_face_keep_refuse_before_launch():
    from customnerf_amd._lib import lib
    org, sp = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    fin = lib.cnerf_tsdf_finalize
    assert fin(FAKE, 8, 8, 1, -1.0, FAKE, FAKE, None) == EINVAL and fin(FAKE, 2048, 2048, 1024, -1.0, FAKE, FAKE, None) == EINVAL
    assert fin(None, 8, 8, 8, -1.0, FAKE, FAKE, None) == ENULL and fin(FAKE, 8, 8, 8, -1.0, None, FAKE, None) == ENULL
    assert fin(FAKE, 8, 8, 8, -1.0, FAKE, None, None) == ENULL
    keep = lambda **k: lib.cnerf_tsdf_face_keep(*[{**dict(state=FAKE, nx=8, ny=8, nz=8, org=org, sp=sp, verts=FAKE, V=3, faces=FAKE, F=1,  # noqa: E731
                                                          keep=FAKE, stream=None), **k}[a] for a in
                                                  ("state", "nx", "ny", "nz", "org", "sp", "verts", "V", "faces", "F", "keep", "stream")])
    assert keep(F=0) == 0 and keep(F=0, state=None, faces=None, keep=None) == 0  # zero faces: no launch
    for k in ("state", "org", "sp", "verts", "faces", "keep"):
        assert keep(**{k: None}) == ENULL, k
    assert keep(nx=1) == EINVAL and keep(F=1 << 31) == EINVAL and keep(V=1 << 31) == EINVAL and keep(nx=2048, ny=2048, nz=1024) == EINVAL


def test_python_side_rejects_before_the_device():
    import torch
    from customnerf_amd import mesh
    from customnerf_amd.nerf.renderer import NeRFRenderer
    assert inspect.signature(NeRFRenderer.extract_mesh).parameters['tsdf'].default is None
    assert 'render_depth' in vars(NeRFRenderer)
    for bad in (dict(shape=(8, 1, 8)), dict(shape=(8, 8)), dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=float("nan")),
                dict(shape=(2048, 2048, 512)), dict(origin=(0, 0)), dict(spacing=(1, 1, 1, 1))):
        with pytest.raises(ValueError):
            mesh.TSDFVolume(**{**dict(shape=(8, 8, 8), origin=(0, 0, 0), spacing=(1, 1, 1), trunc=1.0), **bad})
    with pytest.raises(RuntimeError):
        mesh.TSDFVolume((8, 8, 8), (0, 0, 0), (1, 1, 1), 1.0, device='cpu')
    tv = mesh.TSDFVolume((8, 8, 8), (0, 0, 0), (1, 1, 1), 1.0)
    eye = np.eye(4, dtype=np.float32)
    with pytest.raises(RuntimeError):
        tv.integrate(torch.zeros(4, 4), eye, (1, 1, 2, 2))                       # no CPU path
    with pytest.raises(RuntimeError):
        tv.face_keep(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    assert tv.views == 0 and tv.shape == (8, 8, 8) and tv.trunc == 1.0
    opts = NeRFRenderer._tsdf_options
    good = dict(poses=np.stack([eye, eye]), intrinsics=(1, 1, 2, 2), H=4, W=4)
    cfg = opts(good, False, 'all', 0.25)
    assert cfg['trunc'] == 1.0 and cfg['min_opacity'] == 0.5 and cfg['carve'] is True and cfg['convention'] == 'nerfstudio'
    assert cfg['render'] == {} and tuple(cfg['poses'].shape) == (2, 4, 4)
    with pytest.raises(ValueError):
        opts(good, True, 'all', 0.25)                                            # with sparse=True
    with pytest.raises(ValueError):
        opts(good, False, 'fg', 0.25)
    for k in ("poses", "intrinsics", "H", "W"):
        with pytest.raises(ValueError):
            opts({a: b for a, b in good.items() if a != k}, False, 'all', 0.25)
    for bad in (dict(poses=np.zeros((0, 4, 4), np.float32)), dict(trunc=0.0), dict(trunc=-0.1), dict(colour=True), dict(convention='opencv'),
                dict(intrinsics=(1, 1, 2)), dict(poses=eye)):
        with pytest.raises(ValueError):
            opts({**good, **bad}, False, 'all', 0.25)
    with pytest.raises(ValueError):
        opts([1, 2], False, 'all', 0.25)


# ------------------------------------------------------------------------------------------------ the sphere, on the restatement
EDGE_BOUND = 0.5                                                                 # lattice steps


@pytest.mark.parametrize("kind", ["ray", "z"])
def test_restatement_fuses_the_sphere(kind):
    """Every zero crossing between two observed points lies within EDGE_BOUND steps of the sphere; the crossing cells at the sphere have
    eight observed corners, and every other crossing cell — the shell where "hidden" meets "never observed" — has an unobserved one, so
    that the face rule removes exactly that shell."""
    n, h = T.RES, T.STEP
    state = T.fuse_sphere(kind)
    vol, count = T.finalize(state, T.SHAPE)
    seen = (state[:, 1] > 0).reshape(T.SHAPE)
    assert count == int(seen.sum()) and 0 < count < n ** 3
    ax = np.linspace(-0.5, 0.5, n)
    P = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1)
    worst, sq, crossings = 0.0, [], 0
    for a in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, n - 1), slice(1, n)
        lo, hi = tuple(lo), tuple(hi)
        v0, v1 = vol[lo].astype(np.float64), vol[hi].astype(np.float64)
        cross = seen[lo] & seen[hi] & ((v0 >= 0) != (v1 >= 0))
        t = (0.0 - v0[cross]) / (v1[cross] - v0[cross])
        pos = P[lo][cross] + t[:, None] * (P[hi][cross] - P[lo][cross])
        err = np.abs(np.linalg.norm(pos, axis=1) - T.RADIUS) / h
        worst, crossings = max(worst, float(err.max())), crossings + int(cross.sum())
        sq.append(err ** 2)
    rms = float(np.sqrt(np.concatenate(sq).mean()))
    print(f"{kind}: {crossings} edge crossings, max {worst:.3f} steps, rms {rms:.3f}; observed share {count / n ** 3:.3f}")
    assert crossings > 1000 and worst <= EDGE_BOUND
    inside = vol >= 0
    corners = [(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
    sub = lambda a, c: a[c[0]:n - 1 + c[0], c[1]:n - 1 + c[1], c[2]:n - 1 + c[2]]  # noqa: E731
    n_in = sum(sub(inside, c).astype(int) for c in corners)
    all_seen = np.logical_and.reduce([sub(seen, c) for c in corners])
    crossing = (n_in > 0) & (n_in < 8)
    centre = sub(P, (0, 0, 0)) + 0.5 * h
    at_surface = np.abs(np.linalg.norm(centre, axis=-1) - T.RADIUS) <= 1.5 * h
    assert (crossing & at_surface).sum() > 1000 and (crossing & ~at_surface).sum() > 100
    assert all_seen[crossing & at_surface].all()                                 # no hole at the surface
    assert not all_seen[crossing & ~at_surface].any()                            # the shell goes, whole


def test_restatement_ignores_the_cut_into_calls():
    cams = T.sphere_cameras()
    depth = np.stack([T.sphere_depth(c, 'ray') for c in cams])
    shape, org, sp = (9, 7, 8), (-0.5, -0.4, -0.45), (0.12, 0.13, 0.125)
    whole = T.integrate(np.zeros((504, 2), np.float32), shape, org, sp, 0.3, depth, cams, T.INTRINSICS)
    parts = np.zeros((504, 2), np.float32)
    for s in (slice(0, 5), slice(5, 6), slice(6, 14)):
        T.integrate(parts, shape, org, sp, 0.3, depth[s], cams[s], T.INTRINSICS)
    assert whole[:, 1].max() > 3 and np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
