"""GPU: cnerf_ssim_grad (csrc/metrics.hip) and metrics.ssim_loss / ssim_with_grad against tests/ssim_grad_restatement.py, the float64 torch
restatement of the definition in include/customnerf_hip.h (itself checked in tests/test_ssim_loss_host.py).

Tolerances, derived, not measured.  The kernels accumulate the moments, the three coefficient maps and the transposed filters in float64
and round every gradient element to float32 ONCE: |g - g64| <= 2^-24 |g64| from that rounding, plus the float64 error of ~400 terms of
size <= ~1e3 max|g64| that may cancel (1e-13 max|g64| at most).  The bound asserted is 2^-23 |g64| + 1e-9 max|g64| per image.  float16
inputs widen exactly, so the same bound holds for them; the half gradient autograd returns for a seed of 1024 is one more rounding, to half:
2^-11 relative for a normal result, 2^-25 absolute for a subnormal one, asserted as 2^-10 |1024 g64| + 2^-24.
Shapes: T = 32 is the tile edge; 11 x 11 is one window, 12 x 45 two window tiles in x with a ragged second one (and two pixel tiles), 43 x 43
has 33 x 33 windows (a one-row and a one-column last tile), 75 x 20 three tiles in y."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ssim_grad_restatement as G  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 11, 11, 1), (2, 12, 45, 3), (1, 43, 43, 3), (1, 75, 20, 1)]
KINDS = ["random", "smooth"]


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind, half=False):
    B, H, W, C = shape
    rng = np.random.default_rng(B * 7 + H * 1000 + W * 10 + C + (kind == "smooth"))
    if kind == "random":
        pred, target = rng.random(shape), rng.random(shape)
    else:                                                           # a smooth image and a slightly noisy copy: small variances, s near 1
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        base = 0.5 + 0.3 * np.sin(x / 7.0 + 0.3)[None, :, :, None] * np.cos(y / 5.0)[None, :, :, None] + 0.05 * np.arange(C)[None, None, None, :]
        pred = np.broadcast_to(base, shape) + 0.03 * np.arange(B)[:, None, None, None]
        target = np.clip(pred + 0.02 * rng.standard_normal(shape), 0, 1)
    dt = np.float16 if half else np.float32
    pred, target = pred.astype(dt), target.astype(dt)
    mask = ((rng.random((B, H, W)) < 0.5) * rng.integers(1, 4, (B, H, W))).astype(np.float32)    # nonzero values other than 1 too
    mask[:, 5, 5] = 1.0                                             # every image keeps a counted window
    for a in (pred, target, mask):
        a.setflags(write=False)
    return pred, target, mask


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, masked, half=False):
    pred, target, mask = _inputs(shape, kind, half)
    s, g = G.ssim_and_grad(pred, target, mask if masked else None)
    return s.numpy(), g.numpy()


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()           # (a writable copy: the cached inputs are read-only)


def _sums_of(entry, pred, target, mask):
    """the raw [B, 5] float64 sums straight from the C entry points, and the gradient where there is one"""
    from customnerf_amd._lib import lib, check, ptr, stream, dtype_id, query_u64
    B, H, W, C = pred.shape
    sums = torch.full((B, 5), -7.0, dtype=torch.float64, device="cuda")
    if entry == "metrics":
        ws = torch.empty(max(query_u64(lib.cnerf_image_metrics_workspace_bytes, B, H, W, C) // 8, 1), dtype=torch.float64, device="cuda")
        check(lib.cnerf_image_metrics(ptr(pred), ptr(target), ptr(mask), B, H, W, C, dtype_id(pred), 0, ptr(sums), None, ptr(ws), stream()), "metrics")
        return sums, None
    ws = torch.empty(max(query_u64(lib.cnerf_ssim_grad_workspace_bytes, B, H, W, C) // 8, 1), dtype=torch.float64, device="cuda")
    grad = torch.full((B, H, W, C), float("nan"), dtype=torch.float32, device="cuda")
    check(lib.cnerf_ssim_grad(ptr(pred), ptr(target), ptr(mask), B, H, W, C, dtype_id(pred), ptr(sums), ptr(grad), ptr(ws), stream()), "ssim_grad")
    return sums, grad


def _check_grad(got, want, what):
    """|g - g64| <= 2^-23 |g64| + 1e-9 max|g64|, the maximum per image (module docstring)"""
    got = got.detach().double().cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all(), what
    worst = 0.0
    for i in range(want.shape[0]):
        gmax = np.abs(want[i]).max()
        bound = 2.0 ** -23 * np.abs(want[i]) + 1e-9 * gmax
        err = np.abs(got[i] - want[i])
        if gmax > 0:
            worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (what, i, float(err.max()), float(gmax))
    print(f"{what}: max |g - g64| / bound = {worst:.3f}")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_sums_are_the_metrics_kernels_bit_for_bit(shape, kind, masked):
    pred, target, mask = (_dev(a) for a in _inputs(shape, kind))
    m = mask if masked else None
    a, _ = _sums_of("metrics", pred, target, m)
    b, grad = _sums_of("grad", pred, target, m)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and bool((a[:, 4] > 0).all())
    assert bool(torch.isfinite(grad).all())                         # every element was written
    ah, _ = _sums_of("metrics", pred.half(), target.half(), m)
    bh, _ = _sums_of("grad", pred.half(), target.half(), m)
    assert torch.equal(ah, bh)
    from customnerf_amd import metrics as M
    s, g = M.ssim_with_grad(pred, target, m)
    assert s.dtype == torch.float64 and torch.equal(s, M.image_metrics(pred, target, m)["ssim"]) and torch.equal(g, grad)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_float32_gradient_against_float64(shape, kind, masked):
    from customnerf_amd import metrics as M
    pred, target, mask = (_dev(a) for a in _inputs(shape, kind))
    s64, g64 = _reference(shape, kind, masked)
    s, g = M.ssim_with_grad(pred, target, mask if masked else None)
    assert g.dtype == torch.float32 and tuple(g.shape) == shape
    assert np.abs(s.cpu().numpy() - s64).max() <= 1e-12
    assert np.abs(g64).max() > 0
    _check_grad(g, g64, f"{shape} {kind} masked={masked}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_float16_inputs_and_the_half_gradient(shape, kind):
    from customnerf_amd import metrics as M
    pred, target, mask = (_dev(a) for a in _inputs(shape, kind, True))
    assert pred.dtype == torch.float16
    _, g64 = _reference(shape, kind, True, True)
    _, g = M.ssim_with_grad(pred, target, mask)
    assert g.dtype == torch.float32
    _check_grad(g, g64, f"{shape} {kind} float16")
    assert torch.equal(g, M.ssim_with_grad(pred.float(), target.float(), mask)[1])           # float16 widens exactly
    # the gradient autograd hands back is half, formed from the float32 product: loss_b = 1 - ssim_b, seeded with 1024 per image
    leaf = pred.clone().requires_grad_(True)
    loss = M.ssim_loss(leaf, target, mask, reduction='none')
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (shape[0],)
    loss.backward(torch.full_like(loss, 1024.0))
    assert leaf.grad.dtype == torch.float16 and leaf.grad.shape == leaf.shape
    want = -1024.0 * g64
    assert np.abs(want).max() < 60000.0                                                      # (the inputs keep the reference inside half's range)
    err = np.abs(leaf.grad.double().cpu().numpy() - want)
    bound = 2.0 ** -10 * np.abs(want) + 2.0 ** -24
    print(f"{shape} {kind}: half gradient max err / bound {float((err / bound).max()):.3f}, max |1024 g64| {np.abs(want).max():.3e}")
    assert np.all(err <= bound)


def test_masks_last_tiles_and_an_empty_image():
    from customnerf_amd import metrics as M
    shape = (1, 43, 43, 3)                                          # 33 x 33 windows: window row / column 32 is a tile of its own
    pred, target, _ = _inputs(shape, "random")
    for name, rows, cols in (("last row", slice(37, 38), slice(5, 38)), ("last column", slice(5, 38), slice(37, 38)), ("corner", slice(37, 38), slice(37, 38))):
        mask = np.zeros(shape[:3], np.float32)
        mask[0, rows, cols] = 1.0                                   # centres (37, .): the windows of row 32 only
        s64, g64 = G.ssim_and_grad(pred, target, mask)
        s, g = M.ssim_with_grad(_dev(pred), _dev(target), _dev(mask))
        assert abs(float(s[0]) - float(s64[0])) <= 1e-12
        _check_grad(g, g64.numpy(), name)
        far = np.ones((43, 43), bool)                               # pixels no counted window covers: exactly zero
        far[rows.start - 5:rows.stop + 5, cols.start - 5:cols.stop + 5] = False
        assert float(g[0].abs().amax(-1).cpu()[torch.from_numpy(far)].max()) == 0.0 and float(g.abs().max()) > 0
    # a batch of two, the first image without a counted window
    shape = (2, 12, 45, 3)
    pred, target, mask = _inputs(shape, "random")
    mask = mask.copy()
    mask[0] = 0.0
    p, t, m = _dev(pred), _dev(target), _dev(mask)
    s, g = M.ssim_with_grad(p, t, m)
    _, g64 = G.ssim_and_grad(pred, target, mask)
    assert bool(torch.isnan(s[0])) and not bool(torch.isnan(s[1]))   # (the score itself is what image_metrics reports: nan, count 0)
    assert float(g[0].abs().max()) == 0.0 and bool(torch.isfinite(g).all())
    _check_grad(g, g64.numpy(), "empty image in a batch")
    leaf = p.clone().requires_grad_(True)
    none = M.ssim_loss(leaf, t, m, reduction='none')
    mean = M.ssim_loss(leaf, t, m)
    assert float(none[0].detach()) == 0.0 and float(none[1].detach()) == float(np.float32(1.0 - float(s[1]))) and float(mean.detach()) == float(none[1].detach())
    mean.backward()
    assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad[0].abs().max()) == 0.0 and torch.equal(leaf.grad[1], -g[1])
    # nothing counted anywhere: a loss of 0 with a zero gradient
    z = torch.zeros_like(m)
    leaf.grad = None
    mean = M.ssim_loss(leaf, t, z)
    mean.backward()
    assert float(mean.detach()) == 0.0 and float(M.ssim_loss(leaf, t, z, reduction='none').detach().abs().max()) == 0.0 and float(leaf.grad.abs().max()) == 0.0


def test_reproducible_from_run_to_run():
    from customnerf_amd import metrics as M
    pred, target, mask = (_dev(a) for a in _inputs((2, 12, 45, 3), "random"))
    big = torch.rand(2, 75, 77, 3, generator=torch.Generator().manual_seed(2)).cuda()
    for a, b, m in ((pred, target, mask), (pred, target, None), (big, big.flip(1), None)):
        one, two = M.ssim_with_grad(a, b, m), M.ssim_with_grad(a, b, m)
        assert torch.equal(one[1], two[1]) and torch.equal(one[0], two[0])
    same = M.ssim_with_grad(big, big)                               # identical images: ssim exactly 1
    assert bool((same[0] == 1.0).all()) and bool(torch.isfinite(same[1]).all())


def test_autograd_wiring():
    from customnerf_amd import metrics as M
    pred, target, mask = (_dev(a) for a in _inputs((2, 12, 45, 3), "random"))
    leaf, tgt = pred.clone().requires_grad_(True), target.clone().requires_grad_(True)
    s, g = M.ssim_with_grad(pred, target, mask)
    loss = M.ssim_loss(leaf, tgt, mask)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert abs(float(loss.detach()) - float((1.0 - s).mean())) <= 2.0 ** -23
    loss.backward()
    assert tgt.grad is None                                         # the target gets no gradient
    assert torch.equal(leaf.grad, -g / 2)                           # two counted images: the mean halves, exactly
    # [H, W, C] is a batch of one, and the gradient comes back in that shape; a scaled seed multiplies in float32
    one = pred[1].clone().requires_grad_(True)
    l1 = M.ssim_loss(one, target[1], mask[1])
    (3.0 * l1).backward()
    assert one.grad.shape == one.shape and torch.equal(one.grad, g[1] * -3.0)
    # a non-contiguous prediction (the trainer's is a slice of the composite output)
    wide = torch.zeros(2, 12, 45, 6, device="cuda")
    wide[..., :3] = pred
    wide.requires_grad_(True)
    M.ssim_loss(wide[..., :3], target, mask).backward()
    assert torch.equal(wide.grad[..., :3], -g / 2) and float(wide.grad[..., 3:].abs().max()) == 0.0
    with pytest.raises(ValueError):
        M.ssim_loss(pred[:, :10], target[:, :10])                    # H = 10: below one window
    with pytest.raises(ValueError):
        M.ssim_loss(pred[..., :2], target[..., :2])                  # C = 2
    with pytest.raises(ValueError):
        M.ssim_loss(pred, target.half())
    with pytest.raises(ValueError):
        M.ssim_loss(pred, target, mask[:, :5])
