"""CPU: what the differentiable SSIM loss promises without a GPU.
  * tests/ssim_grad_restatement.py, the float64 torch reference of tests/test_gpu_ssim_loss.py: its map is the NumPy restatement's bit for
    bit, and the closed form of the gradient that the kernels implement (include/customnerf_hip.h) agrees with torch.autograd;
  * cnerf_ssim_grad / _workspace_bytes are declared, exported and bound, and decide their return codes before any launch;
  * the trainer refuses a lambda_dssim step it cannot interpret before it renders anything.
"""
import argparse
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ssim_restatement as R  # noqa: E402
import ssim_grad_restatement as G  # noqa: E402

CASES = [(1, 11, 11, 1), (2, 12, 45, 3), (1, 43, 43, 3)]


def _inputs(B, H, W, C, seed=0):
    rng = np.random.default_rng(seed + 1000 * H + W)
    pred = rng.random((B, H, W, C)).astype(np.float32)
    target = rng.random((B, H, W, C)).astype(np.float32)
    mask = (rng.random((B, H, W)) < 0.6).astype(np.float32)
    mask[:, H // 2, W // 2] = 1.0
    mask[:, 5, 5] = 1.0                                            # at least one counted window per image
    return pred, target, mask


@pytest.mark.parametrize("B, H, W, C", CASES)
def test_restatement_map_is_the_numpy_restatement_bit_for_bit(B, H, W, C):
    pred, target, _ = _inputs(B, H, W, C)
    got = G.ssim_map(G._t64(pred), G._t64(target)).numpy()
    want = R.ssim_map(pred, target)
    assert got.dtype == np.float64 and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("B, H, W, C", CASES)
def test_restatement_ssim_follows_the_mask_rule(B, H, W, C):
    pred, target, mask = _inputs(B, H, W, C)
    for m in (None, mask):
        s, _ = G.ssim_and_grad(pred, target, m)
        want = R.metrics(pred, target, m)["ssim"]
        assert np.abs(s.numpy() - want).max() <= 1e-14
    s, g = G.ssim_and_grad(pred, target, np.zeros_like(mask))
    assert bool(torch.isnan(s).all()) and float(g.abs().max()) == 0.0


@pytest.mark.parametrize("B, H, W, C", CASES)
def test_closed_form_gradient_agrees_with_autograd(B, H, W, C):
    """1e-12 of max|g|: both sides are float64 sums of at most 121 x 3 terms per pixel formed in different orders"""
    pred, target, mask = _inputs(B, H, W, C)
    for m in (mask, None):
        _, auto = G.ssim_and_grad(pred, target, m)
        closed = G.closed_form_grad(pred, target, m)
        gmax = float(auto.abs().max())
        err = float((auto - closed).abs().max())
        print(f"{B}x{H}x{W}x{C} mask={m is not None}: closed form vs autograd {err / gmax:.3e} of max|g| = {gmax:.3e}")
        assert gmax > 0 and err <= 1e-12 * gmax


def test_gradient_is_a_derivative():
    """a central difference of the restated SSIM along a random direction: the autograd gradient is the derivative of what ssim_of computes"""
    pred, target, mask = _inputs(1, 12, 45, 3, seed=4)
    s, g = G.ssim_and_grad(pred, target, mask)
    rng = np.random.default_rng(8)
    v = torch.from_numpy(rng.standard_normal(pred.shape))
    h = 1e-6
    a = G._t64(pred)
    up, _ = G.ssim_of(a + h * v, G._t64(target), mask)
    dn, _ = G.ssim_of(a - h * v, G._t64(target), mask)
    fd = float((up - dn)[0] / (2 * h))
    an = float((g * v).sum())
    assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-3)


# ------------------------------------------------------------------------------------------------ the C ABI
def _header_args(name):
    path = os.path.join(os.path.dirname(HERE), "include", "customnerf_hip.h")
    text = open(path).read()
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/customnerf_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_symbols_are_declared_exported_and_bound():
    from customnerf_amd import _lib
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8
    for name, n in (("cnerf_ssim_grad_workspace_bytes", 5), ("cnerf_ssim_grad", 12)):
        args = _header_args(name)
        assert len(args) == n, args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == n
        fn = getattr(_lib.lib, name)                               # AttributeError if the library does not export it
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n
    # the same leading arguments as cnerf_image_metrics, minus `quantize`, plus the gradient
    names = lambda args: [re.split(r"[\s\*]+", a)[-1] for a in args]
    m, g = names(_header_args("cnerf_image_metrics")), names(_header_args("cnerf_ssim_grad"))
    assert g == [a for a in m if a not in ("quantize", "ssim_map")][:9] + ["grad_unit", "workspace", "stream"]
    from customnerf_amd import metrics as M
    assert callable(M.ssim_loss) and callable(M.ssim_with_grad)


def test_ssim_grad_argument_validation_without_launch():
    from customnerf_amd._lib import lib
    one = ctypes.c_void_p(16)                  # non-NULL, 8-byte aligned dummy, never dereferenced on these paths
    need = ctypes.c_uint64(0)

    def ws(B, H, W, C):
        need.value = 123
        rc = lib.cnerf_ssim_grad_workspace_bytes(B, H, W, C, ctypes.addressof(need))
        return rc, need.value

    def call(pred=one, target=one, mask=None, B=1, H=16, W=16, C=3, dtype=0, sums=one, grad=one, work=one):
        return lib.cnerf_ssim_grad(pred, target, mask, B, H, W, C, dtype, sums, grad, work, None)

    assert call(H=10) == -1 and call(W=10) == -1 and call(H=10, W=10) == -1                 # below one window: refused
    assert call(C=2) == -1 and call(C=0) == -1 and call(C=4) == -1
    assert call(H=65536) == -1 and call(B=65536, C=1) == -1 and call(B=21846, C=3) == -1
    assert call(dtype=7) == -1
    assert call(pred=None) == -2 and call(target=None) == -2 and call(sums=None) == -2 and call(grad=None) == -2 and call(work=None) == -2
    assert call(work=ctypes.c_void_p(20)) == -1 and call(sums=ctypes.c_void_p(20)) == -1     # float64: 8-byte alignment
    assert call(grad=ctypes.c_void_p(18)) == -1
    assert call(B=0, pred=None, sums=None, grad=None, work=None) == 0                       # empty work is accepted without a launch
    assert ws(1, 10, 16, 3)[0] == -1 and ws(1, 16, 10, 3)[0] == -1 and ws(1, 16, 16, 2)[0] == -1
    assert lib.cnerf_ssim_grad_workspace_bytes(1, 16, 16, 3, None) == -2
    # the metrics call's tile partials, then three float64 maps of (H - 10) x (W - 10) per image and channel
    part = ctypes.c_uint64(0)
    for B, H, W, C in ((1, 11, 11, 1), (1, 43, 42, 1), (2, 43, 43, 3), (3, 75, 20, 3), (1, 800, 800, 3)):
        assert lib.cnerf_image_metrics_workspace_bytes(B, H, W, C, ctypes.addressof(part)) == 0
        assert ws(B, H, W, C) == (0, part.value + B * C * 3 * (H - 10) * (W - 10) * 8)
    assert ws(21845, 65535, 65535, 3)[0] == 0                                                # the largest accepted shape: no overflow of the count
    assert ws(21845, 65535, 65535, 3)[1] > 21845 * 3 * 3 * 65525 * 65525 * 8


def test_python_validation():
    from customnerf_amd import metrics as M
    x = torch.zeros(1, 16, 16, 3)
    with pytest.raises(RuntimeError):
        M.ssim_loss(x, x)                                                                   # CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError):
        M.ssim_with_grad(x, x)
    with pytest.raises(TypeError):
        M.ssim_loss(np.zeros((1, 16, 16, 3), np.float32), x)
    with pytest.raises(ValueError):
        M.ssim_loss(x, x, reduction='sum')


# ------------------------------------------------------------------------------------------------ the trainer's refusals
def _stub(**optkw):
    """what ReconTrainer's step methods touch before they validate: nothing but the options (a model of None proves nothing was rendered)"""
    return types.SimpleNamespace(opt=argparse.Namespace(**optkw), model=None, fused_adam=True, scaler=object(), fp16=False)


@pytest.mark.parametrize("method", ["_train_step", "train_step_graphed"])
def test_trainer_refuses_before_rendering(method):
    from customnerf_amd.trainer import ReconTrainer
    step = getattr(ReconTrainer, method)
    N = 16 * 16
    o, d, rgb, mask = torch.zeros(1, N, 3), torch.zeros(1, N, 3), torch.zeros(1, N, 3), torch.zeros(1, N, 1)
    kw = dict(num_steps=8, upsample_steps=8)
    with pytest.raises(ValueError, match="image_hw"):
        step(_stub(lambda_dssim=0.2), o, d, rgb, mask, **kw)                                # missing
    with pytest.raises(ValueError, match="rays"):
        step(_stub(lambda_dssim=0.2), o, d, rgb, mask, image_hw=(16, 15), **kw)             # H W != N
    with pytest.raises(ValueError, match="window"):
        step(_stub(lambda_dssim=0.2), o[:, :160], d[:, :160], rgb[:, :160], mask[:, :160], image_hw=(10, 16), **kw)
    with pytest.raises(ValueError, match="window"):
        step(_stub(lambda_dssim=0.2), o[:, :160], d[:, :160], rgb[:, :160], mask[:, :160], image_hw=(16, 10), **kw)
    with pytest.raises(ValueError, match="image_hw"):
        step(_stub(lambda_dssim=0.2), o, d, rgb, mask, image_hw=16, **kw)
    with pytest.raises(ValueError):
        step(_stub(lambda_dssim=0.2, batch_rays=64), o, d, rgb, mask, image_hw=(16, 16), **kw)


def test_trainer_check_passes_what_it_should():
    from customnerf_amd import trainer as T
    ns = argparse.Namespace
    assert not T.dssim_wanted(ns()) and not T.dssim_wanted(ns(lambda_dssim=0)) and not T.dssim_wanted(ns(lambda_dssim=0.0))
    assert T.dssim_wanted(ns(lambda_dssim=0.2))
    assert T.dssim_check(ns(lambda_dssim=0.2), (16, 16), 256) is None and T.dssim_check(ns(lambda_dssim=0.2, batch_rays=0), (11, 11), 121) is None
    # the option absent or zero: nothing is checked, whatever arrives
    assert T.dssim_check(ns(), None, 7) is None and T.dssim_check(ns(lambda_dssim=0, batch_rays=64), (3, 3), 7) is None
    with pytest.raises(ValueError):
        T.dssim_check(ns(lambda_dssim=0.2), (16, 16), 256, select_inds=[0, 1])
