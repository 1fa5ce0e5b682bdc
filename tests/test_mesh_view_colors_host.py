"""CPU: the C-ABI of cnerf_view_colors_* up to the point where it would launch, the argument checks of mesh.ViewColors, of
extract_mesh(color_views=...) and of save_mesh, and the NumPy restatement of the fusion (tests/view_colors_restatement.py): its edge
cases, its independence of the cut into batches, occlusion, constant colour, and the coloured sphere."""
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
import raster_restatement as RR  # noqa: E402
import view_colors_restatement as V  # noqa: E402

ROOT = os.path.dirname(HERE)
NAMES = ("cnerf_view_colors_accumulate", "cnerf_view_colors_resolve")
EINVAL, ENULL = -1, -2
FAKE = 1 << 20                                                                   # never dereferenced: every call returns before a launch
BITS = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)             # noqa: E731
SPHERE_BOUND = 1.4e-3                                                            # 2 x the measured 6.6e-4 (test_restatement_colours_the_sphere)


def test_abi_declared_bound_and_exported():
    from customnerf_amd import _lib
    src = open(os.path.join(ROOT, "include", "customnerf_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8
    block = src[src.index("Multi-view colour fusion:"):src.index("int cnerf_view_colors_accumulate(")]
    assert "ONE ROUNDING PER WRITTEN OPERATION" in block.upper() and "ALL FOUR" in block


ACC_ARGS = ("points", "normals", "M", "images", "depth", "pw", "n", "H", "W", "c2w", "fx", "fy", "cx", "cy", "conv", "near", "kind", "tol",
            "min_cos", "power", "state", "seen", "stream")


def _accumulate(**k):
    from customnerf_amd._lib import lib
    cam = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    a = dict(points=FAKE, normals=FAKE, M=8, images=FAKE, depth=FAKE, pw=None, n=1, H=4, W=4, c2w=cam, fx=1.0, fy=1.0, cx=2.0, cy=2.0, conv=0,
             near=0.01, kind=0, tol=0.1, min_cos=0.2, power=2, state=FAKE, seen=FAKE, stream=None)
    a.update(k)
    return lib.cnerf_view_colors_accumulate(*[a[n] for n in ACC_ARGS])


@pytest.mark.parametrize("over", [dict(n=17), dict(n=1 << 20), dict(conv=2), dict(conv=-1), dict(kind=2), dict(kind=-1), dict(power=0),
                                  dict(power=9), dict(power=-1), dict(tol=0.0), dict(tol=-1.0), dict(tol=float("inf")), dict(tol=float("nan")),
                                  dict(min_cos=-0.1), dict(min_cos=1.0), dict(min_cos=float("nan")), dict(fx=0.0), dict(fy=0.0),
                                  dict(fx=float("inf")), dict(fy=float("nan")), dict(cx=float("inf")), dict(cy=float("nan")),
                                  dict(near=float("inf")), dict(M=1 << 31), dict(H=1 << 16, W=1 << 15)], ids=str)
def test_accumulate_refuses_before_launch(over):
    assert _accumulate(**over) == EINVAL
    if 'n' not in over:
        assert _accumulate(n=0, **over) == EINVAL                                # also with nothing to do
    if 'M' not in over:
        assert _accumulate(M=0, **over) == EINVAL


def test_accumulate_null_and_empty():
    for k in ("points", "normals", "images", "depth", "c2w", "state", "seen"):
        assert _accumulate(**{k: None}) == ENULL, k
    empty = dict(points=None, normals=None, images=None, depth=None, c2w=None, state=None, seen=None)
    assert _accumulate(M=0) == 0 and _accumulate(M=0, **empty) == 0              # no point: no launch
    assert _accumulate(n=0) == 0 and _accumulate(n=0, **empty) == 0              # no view: no launch
    assert _accumulate(state=None, power=0) == EINVAL                            # the values are looked at first
    assert _accumulate(state=FAKE + 4) == EINVAL                                 # a state row is one 16-byte access
    assert _accumulate(H=1) == 0 and _accumulate(W=1) == 0 and _accumulate(H=0, W=0) == 0     # no 2 x 2 footprint fits: no launch


def test_resolve_refuses_before_launch():
    from customnerf_amd._lib import lib
    fill = (C.c_float * 3)(0, 0, 0)
    res = lambda **k: lib.cnerf_view_colors_resolve(*[{**dict(state=FAKE, seen=FAKE, M=8, fallback=None, fill=fill, out=FAKE, counts=FAKE,  # noqa: E731
                                                               stream=None), **k}[a] for a in
                                                      ("state", "seen", "M", "fallback", "fill", "out", "counts", "stream")])
    for k in ("state", "seen", "fill", "out", "counts"):
        assert res(**{k: None}) == ENULL, k
    assert res(M=1 << 31) == EINVAL and res(state=FAKE + 8) == EINVAL
    assert res(M=0) == 0 and res(M=0, state=None, seen=None, out=None, counts=None) == 0


def test_view_colors_rejects_before_the_device():
    import torch
    from customnerf_amd import mesh
    N, H, W = 3, 6, 8
    eye = np.eye(4, dtype=np.float32)
    good = dict(images=torch.zeros(N, H, W, 3), depth=torch.ones(N, H, W), c2w=np.stack([eye] * N), intrinsics=(5, 5, 4, 3), depth_tol=0.1)
    sig = inspect.signature(mesh.ViewColors.__init__).parameters
    assert sig['depth_tol'].default is inspect.Parameter.empty                   # required: a scale only the caller knows
    assert (sig['power'].default, sig['min_cos'].default, sig['near'].default, sig['depth_kind'].default) == (2, 0.2, 0.01, 'z')
    nan_cam = np.stack([eye] * N)
    nan_cam[1, 0, 3] = np.nan
    for bad in (dict(images=torch.zeros(N, H, W)), dict(images=torch.zeros(N, H, W, 4)), dict(depth=torch.ones(N, H, W + 1)),
                dict(depth=torch.ones(N + 1, H, W)), dict(weights=torch.ones(N, H)), dict(images=torch.zeros(N, H, W, 3, dtype=torch.float64)),
                dict(depth=torch.ones(N, H, W, dtype=torch.float16)), dict(weights=torch.ones(N, H, W, dtype=torch.int32)),
                dict(c2w=np.stack([eye] * 2)), dict(c2w=np.zeros((N, 2, 4), np.float32)), dict(c2w=nan_cam), dict(intrinsics=(5, 5, 4)),
                dict(intrinsics=(0, 5, 4, 3)), dict(intrinsics=(5, float("inf"), 4, 3)), dict(near=float("nan")),
                dict(convention='opencv'), dict(depth_kind='disparity'), dict(depth_tol=0.0), dict(depth_tol=-1.0), dict(depth_tol=float("nan")),
                dict(power=0), dict(power=9), dict(power=2.5), dict(power=True), dict(min_cos=-0.01), dict(min_cos=1.0),
                dict(min_cos=float("nan")), dict(fallback=3), dict(fill=(0, 0)), dict(fill=(0, 0, float("inf")))):
        with pytest.raises(ValueError):
            mesh.ViewColors(**{**good, **bad})
    with pytest.raises(TypeError):
        mesh.ViewColors(**{k: v for k, v in good.items() if k != 'depth_tol'})
    with pytest.raises(RuntimeError):
        mesh.ViewColors(**good)                                                  # everything else is right: there is no CPU path


def test_extract_mesh_options_reject_before_any_render(tmp_path):
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.renderer import NeRFRenderer
    from customnerf_amd.scene import make_opt
    assert inspect.signature(NeRFRenderer.extract_mesh).parameters['color_views'].default is None
    assert 'render_view' in vars(NeRFRenderer)
    eye = np.eye(4, dtype=np.float32)
    good = dict(poses=np.stack([eye, eye]), intrinsics=(1, 1, 2, 2), H=4, W=4)
    opts = NeRFRenderer._color_view_options
    cfg = opts(good, None, True, 0.25)
    assert cfg['depth_tol'] == 0.5 and cfg['power'] == 2 and cfg['min_cos'] == 0.2 and cfg['min_opacity'] == 0.5
    assert cfg['convention'] == 'nerfstudio' and cfg['render'] == {} and tuple(cfg['poses'].shape) == (2, 4, 4)
    assert opts({**good, 'depth_tol': 0.1, 'power': 4, 'min_cos': 0.0}, None, True, 0.25)['depth_tol'] == 0.1
    tsdf = {**good, 'trunc': 1.0, 'convention': 'ngp', 'min_opacity': 0.9, 'carve': False}
    same = opts('tsdf', tsdf, True, 0.25)                                        # the cameras of tsdf=, not its fusion options
    assert same['convention'] == 'ngp' and same['min_opacity'] == 0.9 and 'trunc' not in same and same['depth_tol'] == 0.5
    with pytest.raises(ValueError):
        opts('tsdf', None, True, 0.25)                                           # without tsdf=
    with pytest.raises(ValueError):
        opts(good, None, False, 0.25)                                            # neither color=True nor texture=R
    for k in ("poses", "intrinsics", "H", "W"):
        with pytest.raises(ValueError):
            opts({a: b for a, b in good.items() if a != k}, None, True, 0.25)
    bad_pose = np.stack([eye, eye])
    bad_pose[0, 1, 1] = np.inf
    for bad in (dict(poses=np.zeros((0, 4, 4), np.float32)), dict(poses=eye), dict(poses=bad_pose), dict(depth_tol=0.0), dict(depth_tol=-0.1),
                dict(power=0), dict(power=9), dict(power=1.5), dict(min_cos=1.0), dict(min_cos=-0.5), dict(colour=True),
                dict(convention='opencv'), dict(intrinsics=(1, 1, 2)), dict(H=1), dict(trunc=1.0)):
        with pytest.raises(ValueError):
            opts({**good, **bad}, None, True, 0.25)
    for bad in ([1, 2], 'views', 3):
        with pytest.raises(ValueError):
            opts(bad, tsdf, True, 0.25)
    model = NeRFNetwork(make_opt())                                              # on the host: every check comes before the first launch
    for kw in (dict(color_views=good), dict(color_views='tsdf', color=True), dict(color_views={**good, 'power': 0}, texture=64),
               dict(color_views='nope', color=True)):
        with pytest.raises(ValueError):
            model.extract_mesh(resolution=8, **kw)
    with pytest.raises(ValueError):
        model.save_mesh(str(tmp_path / "m.ply"), resolution=8, color_views=good)                 # needs color=True or texture=R
    with pytest.raises(ValueError):
        model.save_mesh(str(tmp_path / "m.ply"), resolution=8, color_views=good, texture=64)     # PLY carries no texture
    with pytest.raises(ValueError):
        model.save_mesh(str(tmp_path / "m.obj"), resolution=8, color_views={**good, 'min_cos': 2.0}, texture=64)
    assert not os.listdir(tmp_path)


# ------------------------------------------------------------------------------------------------ the restatement's own properties
def fuse(sc, views=slice(None), weights=True, **kw):
    kw = {**dict(convention='nerfstudio', depth_kind='z', power=2, min_cos=V.MIN_COS, near=V.NEAR), **kw}
    return V.fuse(sc['points'], sc['normals'], sc['images'][views], sc['depth'][views], sc['cams'][views], V.K, V.TOL,
                  weights=sc['weights'][views] if weights else None, **kw)


@pytest.mark.parametrize("kind", ["z", "ray"])
@pytest.mark.parametrize("convention", ["nerfstudio", "ngp"])
def test_restatement_edge_cases(convention, kind):
    """view 0 alone, on the points laced into the scene: each case's condition decides (view_colors_restatement.EDGE_CASES)"""
    sc = V.edge_scene(17, convention, kind)
    for weights in (True, False):
        _, seen = fuse(sc, slice(0, 1), weights, convention=convention, depth_kind=kind)
        for name, want in V.EDGE_CASES.items():
            want = 1 if name == 'weight0' and not weights else want
            assert seen[sc['edge'][name]] == want, (name, weights)


def test_restatement_ignores_the_cut_into_batches():
    sc = V.edge_scene(33, 'nerfstudio', 'z')
    whole, seen = fuse(sc)
    state, count = np.zeros((V.NPTS, 4), np.float32), np.zeros(V.NPTS, np.uint32)
    for s in (slice(0, 1), slice(1, 17), slice(17, 18), slice(18, 33)):
        V.accumulate(state, count, sc['points'], sc['normals'], sc['images'][s], sc['depth'][s], sc['cams'][s], V.K, V.TOL,
                     weights=sc['weights'][s], min_cos=V.MIN_COS, near=V.NEAR)
    assert seen.max() >= 4 and np.array_equal(BITS(whole), BITS(state)) and np.array_equal(seen, count)
    out, counts = V.resolve(whole, seen)
    assert counts.sum() == V.NPTS and (counts > 0).all()


def test_restatement_occluder_hides_the_point():
    """a point on the far side of the sphere projects onto the near side's depth: the view adds nothing, with any normal"""
    cam = V.look_at((0, 0, 1.5))[None]
    image, _, z = V.sphere_render(cam[0], V.H, V.W, V.K)
    p = np.array([[0.01, 0.02, -V.RADIUS], [0.01, 0.02, V.RADIUS]], np.float32)  # behind and in front, on one ray (nearly)
    n = np.array([[0, 0, 1], [0, 0, 1]], np.float32)                             # both facing the camera
    assert 2 * V.RADIUS > 10 * V.TOL
    state, seen = V.fuse(p, n, image[None], z[None], cam, V.K, V.TOL)
    assert seen.tolist() == [0, 1] and not state[0].any() and state[1, 3] > 0.9


def test_restatement_returns_a_constant_colour_exactly():
    sc = V.edge_scene(17, 'nerfstudio', 'z')
    # channels that are 0 or a power of two: gx + ax rounds to 1, so the bilinear value is c, and w c, the sums of w c and acc / wsum are
    # exact scalings (any other constant comes back to within a few ulp, not bit for bit)
    for colour in ((0.25, 0.5, 1.0), (1.0, 0.0, 0.125)):
        images = np.broadcast_to(np.array(colour, np.float32), sc['images'].shape)
        state, seen = V.fuse(sc['points'], sc['normals'], images, sc['depth'], sc['cams'], V.K, V.TOL, min_cos=V.MIN_COS, near=V.NEAR)
        out, _ = V.resolve(state, seen, fill=(9.0, 9.0, 9.0))
        assert (seen > 0).sum() > 500
        assert (out[seen > 0] == np.array(colour, np.float32)).all() and (out[seen == 0] == 9.0).all()


def test_resolve_restatement():
    state = np.array([[1, 2, 3, 2], [0, 0, 0, 0], [3, 3, 3, 1.5], [0, 0, 0, 0]], np.float32)
    seen = np.array([1, 0, 5, 0], np.uint32)
    fb = np.arange(12, dtype=np.float32).reshape(4, 3)
    out, counts = V.resolve(state, seen, fb)
    assert out.tolist() == [[0.5, 1, 1.5], [3, 4, 5], [2, 2, 2], [9, 10, 11]] and counts.tolist() == [2, 1, 1]
    out, _ = V.resolve(state, seen, None, (0.1, 0.2, 0.3))
    assert np.array_equal(out[1], np.array([0.1, 0.2, 0.3], np.float32)) and np.array_equal(out[3], out[1])


def test_restatement_colours_the_sphere():
    """Every vertex of the inscribed polyhedron is seen by a view (by two, in fact), and the fused colour lies within SPHERE_BOUND of the
    analytic 0.5 + 0.5 x / |x|.  Measured: max error 6.6e-4 (the bilinear interpolation of 64 x 64 images of a sphere 16 pixels in radius);
    the bound is twice that."""
    verts, faces, normals = V.sphere_mesh()
    cams = V.sphere_cameras()
    depth = np.stack([RR.visibility(verts, faces, c, V.INTRINSICS, V.IMG, V.IMG)['depth'] for c in cams])
    state, seen = V.fuse(verts, normals, V.sphere_images(), depth, cams, V.INTRINSICS, V.SPHERE_TOL)
    out, counts = V.resolve(state, seen)
    err = np.abs(out.astype(np.float64) - V.sphere_color(verts.astype(np.float64))).max()
    print(f"{len(verts)} vertices, seen by {seen.min()} ... {seen.max()} views, max colour error {err:.3e}")
    assert seen.min() >= 1 and counts[0] == 0
    assert err <= SPHERE_BOUND
