"""CPU: the formulas behind the ray regularisers (distortion, ray entropy) hold in float64 — the closed-form gradient chain and the O(S)
prefix-sum form that k_ray_reg_fwd / k_ray_reg_bwd implement equal the definitions' double sum and torch.autograd — and the new entry points
are declared, exported, bound, and validate their arguments before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ray_reg_restatement as rs

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "customnerf_hip.h")


def header_source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def make_case(N=6, num_steps=5, upsample=4, seed=0):
    """sorted samples with a duplicated z, sigma log-uniform over six decades; ray 1 transparent, ray 2 opaque at its first sample, ray 3 misses
    the box (far == near), ray 4 too faint for the entropy gate"""
    g = torch.Generator().manual_seed(seed)
    S = num_steps + upsample
    nears = 0.2 + torch.rand(N, generator=g, dtype=torch.float64)
    fars = nears + 1.0 + torch.rand(N, generator=g, dtype=torch.float64)
    z = (nears[:, None] + (fars - nears)[:, None] * torch.rand(N, S, generator=g, dtype=torch.float64)).sort(1).values
    z[:, 2] = z[:, 1]
    sigma = 10 ** (torch.rand(N, S, generator=g, dtype=torch.float64) * 6 - 3)
    rgbc = torch.rand(N, S, 4, generator=g, dtype=torch.float64) * 0.98 + 0.01
    sigma[1] = 0
    sigma[2, 0] = 1e6
    rgbc[2, 0, 3] = 0.9                     # (inside the edit region: detach_bg must not remove the one sample that carries the ray's gradient)
    z[2, 1] = z[2, 0] + 0.05
    z[2] = z[2].sort().values
    fars[3] = nears[3]
    z[3] = nears[3]
    sigma[4] = 1e-3
    return sigma, rgbc, z, nears, fars, num_steps


@pytest.mark.parametrize("soft", [True, False])
@pytest.mark.parametrize("detach_bg", [False, True])
def test_closed_form_gradient_equals_autograd(soft, detach_bg):
    sigma, rgbc, z, nears, fars, T = make_case()
    g = torch.randn(3, z.shape[0], 2, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    out, gs, gc = rs.regularizers_with_grads(sigma, rgbc, z, nears, fars, T, soft, 0.5, g, detach_bg)
    cs, cc = rs.closed_form_grads(sigma, rgbc, z, nears, fars, T, soft, 0.5, g, detach_bg)
    assert torch.isfinite(out).all() and torch.isfinite(gs).all() and torch.isfinite(gc).all()
    scale = gs.abs().amax(1, keepdim=True).clamp_min(1e-300)
    assert float(((gs - cs).abs() / scale).max()) < 1e-9
    assert float((gc[..., :3]).abs().max()) == 0.0                       # no gradient to rgb
    scale = gc[..., 3].abs().amax(1, keepdim=True).clamp_min(1e-300)
    assert float(((gc[..., 3] - cc).abs() / scale).max()) < 1e-9
    if not soft:
        assert float(gc.abs().max()) == 0.0
    assert float(gs.abs().max()) > 0


def test_prefix_form_equals_double_sum():
    sigma, rgbc, z, nears, fars, T = make_case(seed=3)
    out = rs.regularizers(sigma, rgbc, z, nears, fars, T, True, 0.5)
    sig, c, zz, nn, ff = rs._inputs(sigma, rgbc, z, nears, fars, rs.D)
    for v in range(3):
        w, _, _, delta, hit, L = rs.weights(sig, c[..., 3], zz, nn, ff, T, True, 0.5, v, False, rs.D)
        dist, _ = rs.distortion_prefix(w, delta, L)
        dist = torch.where(hit[:, 0], dist, torch.zeros_like(dist))
        np.testing.assert_allclose(dist.numpy(), out[v, :, 0].numpy(), rtol=1e-11, atol=1e-300)
    assert float(out[0, :, 0].max()) > 1e-3


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_missed_and_gated_rays_are_exact_zeros(dtype):
    sigma, rgbc, z, nears, fars, T = make_case()
    g = torch.ones(3, z.shape[0], 2, dtype=torch.float64)
    out, gs, gc = rs.regularizers_with_grads(sigma, rgbc, z, nears, fars, T, True, 0.5, g, dtype=dtype)
    assert not torch.isnan(out).any() and not torch.isnan(gs).any() and not torch.isnan(gc).any()
    # ray 3: far == near
    assert float(out[:, 3].abs().max()) == 0.0 and float(gs[3].abs().max()) == 0.0 and float(gc[3].abs().max()) == 0.0
    # ray 4 (and the transparent ray 1): weights below min_opacity -> no entropy, and no gradient from it
    assert float(out[:, 4, 1].abs().max()) == 0.0 and float(out[:, 1, 1].abs().max()) == 0.0
    g_ent = torch.zeros(3, z.shape[0], 2, dtype=torch.float64)
    g_ent[..., 1] = 1
    _, gs_e, gc_e = rs.regularizers_with_grads(sigma, rgbc, z, nears, fars, T, True, 0.5, g_ent, dtype=dtype)
    assert float(gs_e[4].abs().max()) == 0.0 and float(gc_e[4].abs().max()) == 0.0 and float(gs_e[1].abs().max()) == 0.0
    assert float(gs_e[0].abs().max()) > 0                                  # an ordinary ray does get one
    assert float(out[0, 0, 1]) > 0
    # with the gate open the faint ray reports its entropy
    assert float(rs.regularizers(sigma, rgbc, z, nears, fars, T, True, 0.5, min_opacity=1e-6, dtype=dtype)[0, 4, 1]) > 0


def test_new_symbols_declared_exported_and_bound():
    from customnerf_amd import _lib
    src = header_source()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cnerf_ray_reg_forward", "cnerf_ray_reg_backward"):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(m.group(1).split(","))
    assert _lib.lib.cnerf_abi_version() == 8


def test_argument_validation_without_launch():
    from customnerf_amd._lib import lib
    one = ctypes.c_void_p(16)             # non-NULL dummy, never dereferenced: every call below returns before a launch

    def fwd(S=8, T=4, vm=1, N=4, **null):
        a = {k: (None if k in null else one) for k in ("sigmas", "rgbc", "z", "nears", "fars", "out")}
        return lib.cnerf_ray_reg_forward(a["sigmas"], a["rgbc"], a["z"], a["nears"], a["fars"], N, S, T, 1, 0.5, None, vm, 0.1, a["out"], None)

    def bwd(S=8, T=4, vm=1, N=4, g_rgbc=None, **null):
        a = {k: (None if k in null else one) for k in ("g", "sigmas", "rgbc", "z", "nears", "fars", "gs")}
        return lib.cnerf_ray_reg_backward(a["g"], a["sigmas"], a["rgbc"], a["z"], a["nears"], a["fars"], N, S, T, 1, 0.5, 0, None, vm, 0.1, a["gs"], g_rgbc,
                                          None)
    for f in (fwd, bwd):
        assert f(S=0) == -1 and f(S=257) == -1 and f(T=0) == -1 and f(vm=0) == -1 and f(vm=8) == -1
        assert f(N=0) == 0                                              # empty work is accepted without a launch
        assert f(N=1 << 30, S=256) == -1                                # row indices are 32-bit
        for k in ("sigmas", "rgbc", "z", "nears", "fars"):
            assert f(**{k: True}) == -2, k
    assert fwd(out=True) == -2 and bwd(g=True) == -2 and bwd(gs=True) == -2
    assert bwd(g_rgbc=ctypes.c_void_p(24)) == -1                        # the confidence gradient is written as float4


def test_run_cuda_rejects_ray_reg():
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.scene import make_opt
    model = NeRFNetwork(make_opt(cuda_ray=True, num_levels=4))
    o = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError, match="ray_reg"):
        model.run_cuda(o, o, ray_reg=True)
    with pytest.raises(ValueError, match="ray_reg"):
        model.render(o, o, ray_reg=True)
