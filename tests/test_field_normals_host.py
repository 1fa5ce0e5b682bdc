"""CPU: the field-normal restatement (tests/field_normal_restatement.py) pinned to the C oracle and to central differences, the three new
entry points' declarations and argument checks, and the Python surface's refusals.  No GPU compute is issued here."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import field_normal_restatement as FN
from oracle import c_oracle as co
from oracle import torch_oracle as to

NEW = ("cnerf_field_density_grad", "cnerf_grid_encode_input_grad", "cnerf_composite_normals")
EINVAL = -1


def small_grid(gridtype, L=6, log2_T=12, finest=256, seed=0, half=False):
    offsets, pls = to.grid_offsets(3, L, 2, 2, 16, log2_T, finest)
    g = torch.Generator().manual_seed(seed)
    table = (torch.rand(int(offsets[-1]), 2, generator=g) * 2 - 1) * 0.5
    if half:
        table = table.half().float()
    return offsets, pls, table, {'hash': 0, 'tiled': 1}[gridtype]


def edge_points(n, seed, scale0):
    """uniform points plus the edge cases: coordinates exactly 0 and exactly 1, nodes of the coarsest level, points outside [0, 1]"""
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3)).astype(np.float32)
    x[0] = (0.0, 0.3, 0.7)
    x[1] = (1.0, 1.0, 1.0)
    x[2] = (0.0, 0.0, 0.0)
    x[3] = (0.25, 1.0, 0.0)
    for k in range(4):                                                # pos = x scale + 0.5 is an integer: a grid node of level 0
        x[4 + k] = (np.float32((k + 1 - 0.5) / scale0), np.float32((2 * k + 2 - 0.5) / scale0), x[4 + k, 2])
    x[8] = (-0.01, 0.5, 0.5)
    x[9] = (0.5, 1.0000001, 0.5)
    x[10] = (0.5, 0.5, 7.0)
    return x


@pytest.mark.parametrize("gridtype", ["hash", "tiled"])
def test_restatement_equals_the_c_oracle(gridtype):
    """features and dy_dx of the restatement (float32-faithful cells) against oracle.c_oracle.grid_encode_forward(calc_grad_inputs=True), to
    float32 rounding: 8 products of <= 4 factors and 7 additions per value, i.e. 16 x 2^-23 of the largest possible magnitude per level"""
    offsets, pls, table, gt = small_grid(gridtype)
    lv = FN.levels(offsets, pls, 16)
    x = edge_points(300, 1, lv[0][2])
    ok = FN.in_range(torch.from_numpy(x)).numpy()
    out, dy = co.grid_encode_forward(x, table.numpy(), offsets, pls, 16, True, gt, False, 0)
    L = len(lv)
    f = FN.grid_features(torch.from_numpy(x).double(), table.double(), offsets, pls, 16, gt).numpy()
    d = FN.grid_dy_dx(torch.from_numpy(x).double(), table.double(), offsets, pls, 16, gt).numpy()
    tmax = float(table.abs().max())
    assert np.abs(out.reshape(-1, L, 2) - f).max() <= 16 * 2.0 ** -23 * tmax
    dy = dy.reshape(-1, L, 3, 2)
    for l in range(L):
        assert np.abs(dy[:, l] - d[:, l]).max() <= 16 * 2.0 ** -23 * tmax * lv[l][2], l
    assert not ok[8:11].any() and ok[:8].all()
    assert (f[8:11] == 0).all() and (d[8:11] == 0).all() and np.abs(d[:8]).max() > 0


@pytest.mark.parametrize("gridtype", ["hash", "tiled"])
def test_restatement_derivative_equals_central_differences(gridtype):
    """plain float64 function, points at least 0.1 of a cell away from every cell face on every level: the interpolant is linear along each
    axis inside a cell, so central differences are exact up to float64 rounding; autograd and the explicit derivative agree with them"""
    offsets, pls, table, gt = small_grid(gridtype, L=5, finest=128)
    lv = FN.levels(offsets, pls, 16)
    rng = np.random.default_rng(4)
    pts = []
    while len(pts) < 40:
        c = rng.random(3)
        fr = np.array([(c * s + 0.5) % 1.0 for _, _, s, _ in lv])
        if fr.min() > 0.1 and fr.max() < 0.9:
            pts.append(c)
    x = torch.tensor(np.array(pts), dtype=torch.float64)
    tab = table.double()
    feats = lambda y: FN.grid_features(y, tab, offsets, pls, 16, gt, fp32_cell=False)          # noqa: E731
    h = 1e-5
    cd = torch.zeros(len(pts), len(lv), 3, 2, dtype=torch.float64)
    for d in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[d] = h
        cd[:, :, d] = (feats(x + e) - feats(x - e)) / (2 * h)
    dy = FN.grid_dy_dx(x, tab, offsets, pls, 16, gt, fp32_cell=False)
    scale = float(dy.abs().max())
    assert scale > 1 and float((dy - cd).abs().max()) <= 1e-9 * scale
    g_enc = torch.from_numpy(rng.standard_normal((len(lv), len(pts), 2)))
    xr = x.clone().requires_grad_(True)
    (ga,) = torch.autograd.grad((feats(xr) * g_enc.permute(1, 0, 2)).sum(), xr)
    ge, ab = FN.grid_input_grad(x, tab, offsets, pls, 16, g_enc, gt, fp32_cell=False)
    assert float((ga - ge).abs().max()) <= 1e-12 * float(ab.max()) and bool((ab >= ge.abs() - 1e-12).all())
    # the float32-faithful cell has the same derivative as long as the cell is the same
    ge32, _ = FN.grid_input_grad(x.float().double(), tab, offsets, pls, 16, g_enc, gt, fp32_cell=True)
    assert float((ge32 - ge).abs().max()) <= 1e-3 * float(ab.max())


def test_restatement_mlp_gradient_and_margin():
    """d raw / d enc of the restatement against central differences of the oracle's forward, away from the ReLU kinks; the half-rounded
    variant keeps the masks of its own forward"""
    ref = to.FieldRef(num_levels=4, n_hidden_geo=2, seed=3)
    g = torch.Generator().manual_seed(1)
    enc = (torch.rand(64, 8, generator=g) * 2 - 1) * 0.5
    raw, grad, margin, zmax = FN.raw_and_grad(enc, ref.network, ref.density_network, 8, 2)
    f = lambda e: to.mlp_forward(to.mlp_forward(e, ref.network.detach().double(), 8, 64, 64, 2), ref.density_network.detach().double(), 64, 1, 64, 1)[:, 0]  # noqa: E731
    h = 1e-7
    keep = margin > 1e-4 * zmax                                      # a step of h moves a pre-activation by far less
    assert keep.float().mean() > 0.5
    for k in range(8):
        e = torch.zeros(8, dtype=torch.float64)
        e[k] = h
        cd = (f(enc.double() + e) - f(enc.double() - e)) / (2 * h)
        assert float((cd - grad[:, k])[keep].abs().max()) <= 1e-6 * float(grad.abs().max())
    raw_h, grad_h, _, _ = FN.raw_and_grad(enc, ref.network, ref.density_network, 8, 2, half=True)
    assert grad_h.dtype == torch.float32 and float((raw_h - raw).abs().max()) < 2e-2
    rel = ((grad_h.double() - grad).norm(dim=-1) / grad.norm(dim=-1)).median()
    assert float(rel) < 1e-2


def test_restatement_composite():
    w = torch.rand(2, 3, 5)
    gx = torch.randn(15, 3)
    gx[4] = 0
    d = torch.randn(3, 3)
    nm, orient = FN.composite_normals(w, None, gx, d)
    n = -gx / gx.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    n[4] = 0
    want = (w.double()[..., None] * n.double().view(1, 3, 5, 3)).sum(2)
    assert torch.allclose(nm, want, atol=1e-6) and tuple(orient.shape) == (2, 3) and bool((orient >= 0).all())


# ------------------------------------------------------------------------------------------------ the C ABI
def header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "customnerf_hip.h")).read()


def test_entry_points_are_declared_bound_and_the_abi_stays_8():
    from customnerf_amd import _lib
    raw = header()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define\s+CNERF_ABI_VERSION\s+8\b", raw)
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.lib, name)


def test_unsupported_shapes_are_einval_before_any_launch():
    from customnerf_amd._lib import lib, F32, F16
    offs = np.arange(0, 8 * 41, 8, dtype=np.int32)                   # 40 levels' worth of offsets
    o = offs.ctypes.data

    def gig(D=3, C=2, L=16, gridtype=0, align=0, interp=0, dtype=F32, B=0):
        return lib.cnerf_grid_encode_input_grad(None, None, o, None, None, B, D, C, L, 1.0, 16, gridtype, align, interp, dtype, 0, None)
    assert gig() == 0 and gig(dtype=F16, gridtype=1, L=32) == 0       # B = 0: accepted, nothing to do
    for bad in (dict(D=2), dict(D=4), dict(C=1), dict(C=4), dict(interp=1), dict(align=1), dict(L=33), dict(L=0), dict(gridtype=2), dict(dtype=7)):
        assert gig(**bad) == EINVAL, bad
    assert gig(B=5) == -2                                             # the right shape, NULL pointers

    def fdg(enc_dim=32, n_geo=2, dtype=F32, P=0):
        return lib.cnerf_field_density_grad(None, None, P, enc_dim, n_geo, None, None, None, None, dtype, 0, None)
    assert fdg() == 0 and fdg(enc_dim=64, n_geo=1, dtype=F16) == 0
    for bad in (dict(enc_dim=66), dict(enc_dim=0), dict(enc_dim=7), dict(n_geo=3), dict(n_geo=0), dict(dtype=2)):
        assert fdg(**bad) == EINVAL, bad
    assert fdg(P=3) == -2
    cn = lambda V, N=0, S=4: lib.cnerf_composite_normals(None, None, None, None, V, N, S, 0, None, None, None)      # noqa: E731
    assert cn(1) == 0 and cn(3) == 0 and cn(0) == EINVAL and cn(4) == EINVAL and cn(1, S=0) == EINVAL and cn(1, N=2) == -2


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_surface_refusals(tmp_path):
    from customnerf_amd import tcnn
    from customnerf_amd.field import field_density_grad
    from customnerf_amd.gridencoder import GridEncoder
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.renderer import NeRFRenderer
    from customnerf_amd.scene import make_opt
    sig = inspect.signature
    assert list(sig(field_density_grad).parameters) == ['enc', 'xyz', 'enc_dim', 'n_hidden_geo', 'p_net', 'p_den', 'enc_level_stride', 'want_sigma']
    assert list(sig(GridEncoder.input_grad).parameters)[:4] == ['self', 'unit', 'grad_enc', 'level_stride']
    assert sig(NeRFRenderer.run).parameters['normals'].default is False
    assert sig(NeRFRenderer.extract_mesh_normals).parameters['normals'].default == 'field'
    from customnerf_amd.nerf import mesh_export
    assert mesh_export.VIEW_OPTIONS == {'normals': False, 'shading': None, 'light_d': None, 'ambient_ratio': 0.1, 'path': None}
    assert sig(mesh_export.parse_options).parameters['normals'].default == 'mesh'
    model = NeRFNetwork(make_opt(num_levels=4, n_hidden_geo=1))       # on the host
    x = torch.zeros(5, 3)
    for fn in (model.density_gradient, model.normal):
        with pytest.raises(NotImplementedError, match="CUDA"):
            fn(x)
    unfused = NeRFNetwork(make_opt(num_levels=4, n_hidden_geo=1, fused_field=False))
    for fn in (unfused.density_gradient, unfused.normal):
        with pytest.raises(NotImplementedError, match="fused"):
            fn(x)
    march = NeRFNetwork(make_opt(num_levels=4, n_hidden_geo=1, cuda_ray=True))
    with pytest.raises(NotImplementedError, match="run_cuda"):
        march.run_cuda(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), normals=True)
    eye = np.eye(4, dtype=np.float32)
    cams = dict(poses=np.stack([eye, eye]), intrinsics=(1, 1, 2, 2), H=4, W=4)
    for kw in (dict(normals='field', part='fg'), dict(normals='field', part='bg'), dict(normals='field', tsdf=cams),
               dict(normals='field', remesh=16), dict(normals='vertex'), dict(normals=True)):
        with pytest.raises(ValueError):
            model.extract_mesh_normals(resolution=8, **kw)
    with pytest.raises(TypeError):
        model.extract_mesh_normals(resolution=8, colour=True)          # an unknown option, as extract_mesh refuses it
    for kw in (dict(shading='phong'), dict(shading='lambertian', ambient_ratio=1.5)):
        with pytest.raises(ValueError):
            model.render_view(eye, (1, 1, 2, 2), 4, 4, **kw)
    with pytest.raises(ValueError):
        model.save_mesh(str(tmp_path / "m.ply"), resolution=8, normals='field', part='fg')
    assert not list(tmp_path.iterdir())
    assert tcnn is not None
