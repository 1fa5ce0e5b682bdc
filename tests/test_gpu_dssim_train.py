"""GPU: opt.lambda_dssim on the reconstruction trainer — loss = recon_loss + lambda_dssim * (1 - SSIM) of the rendered view
(trainer.dssim_loss -> metrics.ssim_loss -> cnerf_ssim_grad) — on tiny fused-field scenes of customnerf_amd.scene.

Two sizes.  16 x 16 rays with 8 + 8 samples is the small scene of the tolerance-based checks.  Every check that compares BITS runs at 64 x 64
rays instead: 64 * 64 * 16 samples * 16 levels = 2^20 (sample, level) pairs is where the grid scatter takes its path without float atomics,
whose sums are reproducible (below it the table gradient depends on the order the atomics land in, with or without this feature).

What float32 cannot promise.  The half-precision trainer is bit-reproducible at that size; the float32 one is not, with or without this
feature: two identical float32 runs of the unchanged step (no lambda_dssim anywhere) gave the same losses and the same three MLP gradients,
but table gradients 6.4e-12 apart after one backward (7.3e-12 at 96 x 96), a table 7.5e-7 apart after one optimiser step and 5.9e-3 after
three, the MLP parameters 4.5e-8 apart from the second step on (measured on an MI355X).  So the float32 cases compare bit for bit exactly
what the float32 path reproduces — the first step's loss and image, the MLP gradients, the MLP parameters after one step — and the table
only loosely; the half-precision cases compare everything bit for bit, over all three steps."""
import argparse
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

LAM = 0.2
STEPS = 8                                   # num_steps = upsample_steps
KW = dict(num_steps=STEPS, upsample_steps=STEPS, dt_gamma=0, max_steps=1024)


def _scene(hw, V=1, sphere=False):
    from customnerf_amd import scene as sc
    from customnerf_amd.nerf.provider_utils import generate_rays
    H = W = hw
    c2w = torch.from_numpy(sc.poses(max(V, 2))[:V]).cuda()
    o, d = generate_rays(c2w, *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
    o, d = o.view(V, 1, H * W, 3), d.view(V, 1, H * W, 3)
    if sphere:
        rgb, mask = sc.sphere_targets(o.view(V, H * W, 3), d.view(V, H * W, 3))
    else:
        rgb, mask = sc.targets(V, H, W)
    rgb, mask = rgb.cuda(), mask.cuda()
    return [(o[v].contiguous(), d[v].contiguous(), rgb[v].contiguous(), mask[v].contiguous()) for v in range(V)]


def _trainer(fp16, seed=0, loss_only=None, **optkw):
    """loss_only: options that only the trainer's loss sees (the model keeps its own, e.g. a train_conf that makes the renderer fill its dict)"""
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16 if fp16 else torch.float32)
    torch.manual_seed(seed)
    opt = sc.make_opt(fp16=fp16, num_steps=STEPS, upsample_steps=STEPS, iters=100, **optkw)
    model = NeRFNetwork(opt).cuda()
    topt = argparse.Namespace(**dict(vars(opt), **loss_only)) if loss_only else opt
    return ReconTrainer(model, topt, fp16=fp16), model, topt


DSSIM_ONLY = dict(train_rgb=0.0, train_conf=0.0)        # the compositing loss's own gradient: exact zeros


def _params(model):
    return [p.detach().clone() for p in model.parameters()]


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    from customnerf_amd import tcnn
    yield
    tcnn.set_default_dtype(torch.float16)


# ------------------------------------------------------------------------------------------------ the option absent or zero
@pytest.mark.parametrize("fp16", [True, False])
def test_option_absent_or_zero_is_the_step_as_it_was(fp16, monkeypatch):
    """a trainer whose options never heard of lambda_dssim, one with lambda_dssim = 0 and one with it 0 that is also handed image_hw: the
    same step, and the loss kernel is never reached.  fp16: three steps, every parameter byte for byte.  float32 (module docstring): the first
    step's loss and image and the MLP parameters after it byte for byte; the table within 2 lr of the grid group — Adam's first update is
    lr m / (sqrt(v) + 1e-15) = +-lr whatever the gradient's size, so an entry whose atomically summed gradient lands on either side of zero
    moves by up to 2 lr between two runs of the very same code."""
    from customnerf_amd import metrics as M
    view = _scene(64)[0]

    def boom(*a, **k):
        raise AssertionError("ssim_loss was called with the option off")
    monkeypatch.setattr(M, "ssim_loss", boom)
    results = []
    for variant in ("absent", "zero", "zero+hw"):
        tr, model, opt = _trainer(fp16, **({} if variant == "absent" else {"lambda_dssim": 0}))
        assert hasattr(opt, "lambda_dssim") == (variant != "absent")
        torch.manual_seed(11)
        losses = []
        for i in range(3 if fp16 else 1):
            loss, out = tr.train_step(*view, **KW, **({"image_hw": (64, 64)} if variant == "zero+hw" else {}))
            losses.append(float(loss))
            if i == 0:
                image = out['image'].detach().clone()
        results.append((losses, dict((n, p.detach().clone()) for n, p in model.named_parameters()), sorted(k for k in out.keys()), image,
                        max(g['lr'] for g in tr.optimizer.param_groups)))
    for losses, params, keys, image, lr in results[1:]:
        assert losses == results[0][0] and keys == results[0][2] and torch.equal(image, results[0][3])
        for name, p in params.items():
            if fp16 or name != "pos_en.embeddings":
                assert torch.equal(p, results[0][1][name]), name
            else:
                gap = float((p - results[0][1][name]).abs().max())
                print(f"float32 table after one step: max |diff| between two trainers {gap:.3e} (2 lr = {2 * lr:.3e})")
                assert gap <= 2 * lr
    assert all(np.isfinite(results[0][0]))


# ------------------------------------------------------------------------------------------------ the loss value
@pytest.mark.parametrize("fp16", [True, False])
def test_loss_is_recon_plus_weighted_dssim(fp16):
    """|loss - (recon + 0.2 (1 - ssim))| <= 2^-23: all three float32 values are below 1, so (1 - ssim) rounded to float32, its product with 0.2
    and the sum are each within 2^-25 of exact.  recon comes from a twin trainer without the option (same seeds, so the same first render) and
    ssim from image_metrics on the image the step returned."""
    from customnerf_amd import metrics as M
    view = _scene(16)[0]
    o, d, rgb, mask = view
    tr_a, model_a, _ = _trainer(fp16, lambda_dssim=LAM)
    tr_b, model_b, _ = _trainer(fp16)
    assert all(torch.equal(a, b) for a, b in zip(_params(model_a), _params(model_b)))
    torch.manual_seed(5)
    loss_a, out_a = tr_a.train_step(*view, image_hw=(16, 16), **KW)
    torch.manual_seed(5)
    loss_b, out_b = tr_b.train_step(*view, **KW)
    assert torch.equal(out_a['image'], out_b['image'])
    assert sorted(out_a.keys()) == sorted(out_b.keys())                       # the term adds no key to the result
    ssim = float(M.image_metrics(out_a['image'].detach().reshape(1, 16, 16, 3).float(), rgb.reshape(1, 16, 16, 3))['ssim'][0])
    want = float(loss_b) + LAM * (1.0 - ssim)
    print(f"fp16={fp16}: loss {float(loss_a):.8f}, recon {float(loss_b):.8f}, ssim {ssim:.8f}, recon + 0.2 (1 - ssim) {want:.8f}")
    assert loss_a.dtype == torch.float32 and 0 < float(loss_b) < 1 and float(loss_a) < 1
    assert abs(float(loss_a) - want) <= 2.0 ** -23
    moved = max(float((a - b).abs().max()) for a, b in zip(_params(model_a), _params(model_b)))
    assert moved > 0 and all(bool(torch.isfinite(p).all()) for p in model_a.parameters())


# ------------------------------------------------------------------------------------------------ parameter gradients
def _backward(tr, model, view, draws, loss_of):
    """one render with recorded draws, loss_of(outputs) backward, -> the parameter gradients (the trainer's persistent .grad views, zeroed first)"""
    o, d, rgb, mask = view
    for p in model.parameters():
        p.grad.zero_()
    model.train()
    with torch.autocast('cuda', dtype=torch.float16, enabled=tr.fp16):
        out = model.render(o, d, staged=False, perturb=True, force_all_rays=True, _draws=draws, num_steps=STEPS, upsample_steps=STEPS)
        loss = loss_of(out)
    if tr.scaler is not None:
        tr.scaler.backward(loss)
    else:
        loss.backward()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}, out


def _draws(hw, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return dict(z=torch.rand(hw * hw, STEPS, device="cuda", generator=g), u=torch.rand(hw * hw, STEPS, device="cuda", generator=g))


# max |grad - injected| / max |injected| per parameter tensor, measured on an MI355X.  The bound is 8 x the largest.
MEASURED_GRAD_GAP = {"pos_en.embeddings": 8.453e-07, "network.params": 1.961e-06, "density_network.params": 3.624e-05, "rgb_network.params": 3.011e-07}
GRAD_GAP_BOUND = 8 * max(MEASURED_GRAD_GAP.values())


def test_parameter_gradients_follow_the_float64_restatement():
    """train_rgb = train_conf = 0 in the trainer's options (the model keeps its train_conf: without one the renderer returns an empty dict, as
    the reference does): the compositing loss contributes exact zeros and the D-SSIM term is the only live gradient (the case
    tests/test_gpu_ray_reg.py guards for the regulariser).  Reference: the same render, the loss replaced by <image, G> with G the float64
    restatement's gradient of 0.2 (1 - ssim) at the rendered image, cast to float32 — everything downstream of the image is the same code.
    The bound is 8 x the largest gap measured per parameter tensor (GRAD_GAP_BOUND below, the measured values beside it)."""
    hw = 16
    view = _scene(hw)[0]
    rgb = view[2]
    tr, model, opt = _trainer(False, lambda_dssim=LAM, loss_only=DSSIM_ONLY)
    assert getattr(model.opt, 'early_termination', True) and opt.train_rgb == 0 and opt.train_conf == 0 and model.opt.train_conf > 0
    draws = _draws(hw)
    got, out = _backward(tr, model, view, draws, lambda o: tr.loss(o, rgb, view[3], (hw, hw)))
    img = out['image'].detach().reshape(1, hw, hw, 3)
    _, g64 = G.ssim_and_grad(img, rgb.reshape(1, hw, hw, 3))
    inject = (-LAM * g64).to(torch.float32).cuda().reshape(out['image'].shape)
    want, _ = _backward(tr, model, view, draws, lambda o: tr.recon_loss(o, rgb, view[3]) + (o['image'].float() * inject).sum())
    worst = 0.0
    for name in got:
        gmax = float(want[name].abs().max())
        gap = float((got[name] - want[name]).abs().max()) / gmax if gmax > 0 else float(got[name].abs().max())
        worst = max(worst, gap)
        print(f"{name}: max |grad| {gmax:.3e}, max |diff| / max |grad| {gap:.3e}")
        assert bool(torch.isfinite(got[name]).all())
    assert float(want["pos_en.embeddings"].abs().max()) > 0 and float(want["rgb_network.params"].abs().max()) > 0
    assert worst <= GRAD_GAP_BOUND, worst


@pytest.mark.parametrize("fp16", [True, False])
def test_early_termination_does_not_change_the_gradients(fp16):
    """the D-SSIM gradient and the compositing loss's (zero here) are summed by autograd BEFORE the one compositing backward, so the dead-tile
    flags it raises describe the gradient the field backward gets: with opt.early_termination off, the same bits (64 x 64: module docstring).
    float32 (where the flags are not raised at all: they exist for the half-precision field): the MLP gradients bit for bit; the table
    gradient is not reproducible there between two runs of the same code (module docstring), so it is only held to 1e-3 of its maximum, a
    sanity bound far above the 6e-12 measured between identical runs and far below any real difference."""
    hw = 64
    view = _scene(hw)[0]
    rgb = view[2]
    tr, model, opt = _trainer(fp16, lambda_dssim=LAM, loss_only=DSSIM_ONLY)
    draws = _draws(hw)
    grads = {}
    try:
        for et in (True, False, True):
            model.opt.early_termination = et
            grads.setdefault(et, []).append(_backward(tr, model, view, draws, lambda o: tr.loss(o, rgb, view[3], (hw, hw)))[0])
    finally:
        model.opt.early_termination = True
    if fp16:
        assert model._fused_cfg() and model._half()
    for name in grads[True][0]:
        on, on_again, off = grads[True][0][name], grads[True][1][name], grads[False][0][name]
        assert bool(torch.isfinite(on).all())
        if fp16 or name != "pos_en.embeddings":
            assert torch.equal(on, on_again), name                                      # (reproducible at all: the comparison means something)
            assert torch.equal(on, off), name
        else:
            gmax = float(on.abs().max())
            print(f"float32 table gradient: max |grad| {gmax:.3e}, on/on {float((on - on_again).abs().max()):.3e}, on/off {float((on - off).abs().max()):.3e}")
            assert float((on - off).abs().max()) <= 1e-3 * gmax
    assert float(grads[True][0]["pos_en.embeddings"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ the graphed step
def test_graphed_step_with_the_term():
    hw, V = 64, 2
    views = _scene(hw, V)

    def run(steps=10):
        tr, model, _ = _trainer(True, lambda_dssim=LAM)
        torch.manual_seed(7)
        losses = [float(tr.train_step_graphed(*views[i % V], image_hw=(hw, hw), **KW)[0]) for i in range(steps)]
        return losses, _params(model), tr
    l1, p1, tr = run()
    l2, p2, _ = run()
    assert len(tr._graphs) == V and tr.global_step == 10 + 2 * V
    assert all(k[-1] == (hw, hw) for k in tr._graphs)                                   # image_hw is part of the cache key
    assert l1 == l2 and all(torch.equal(a, b) for a, b in zip(p1, p2))
    assert all(np.isfinite(l1)) and l1[-1] < l1[0], l1
    with pytest.raises(ValueError):
        tr.train_step_graphed(*views[0], **KW)                                           # the option is set: image_hw is required
    with pytest.raises(ValueError):
        tr.train_step_graphed(*views[0], image_hw=(hw, hw + 1), **KW)


# ------------------------------------------------------------------------------------------------ what the term buys
def test_training_with_the_term_raises_ssim():
    """40 float32 steps on one view of the analytic sphere, the same seeds with and without the term; the score is image_metrics on an
    evaluation render, not the code under test"""
    from customnerf_amd import metrics as M
    hw = 16
    view = _scene(hw, sphere=True)[0]
    o, d, rgb, mask = view
    scores = {}
    for lam in (0.0, LAM):
        tr, model, opt = _trainer(False, lambda_dssim=lam, lr=5e-3)
        torch.manual_seed(13)
        for _ in range(40):
            tr.train_step(*view, image_hw=(hw, hw), **KW)
        model.eval()
        img = tr._render_eval(model, o, d)['image'].reshape(1, hw, hw, 3).float()
        m = M.image_metrics(img, rgb.reshape(1, hw, hw, 3))
        scores[lam] = (float(m['ssim'][0]), float(m['psnr'][0]))
    print(f"after 40 steps: ssim / psnr without the term {scores[0.0]}, with lambda_dssim = {LAM} {scores[LAM]}")
    assert np.isfinite(scores[LAM][0]) and scores[LAM][0] > scores[0.0][0]
