"""GPU: the ray regularisers (distortion loss, ray entropy; k_ray_reg_fwd / k_ray_reg_bwd) against the float64 restatement of their
definitions (tests/ray_reg_restatement.py), their determinism and indexing, and their way through the renderer, the early-termination
hand-over of the field backward and the two trainers."""
import argparse
import copy
import functools

import numpy as np
import pytest
import torch

import ray_reg_restatement as rs

# Tolerance of the comparison against float64: per ray, relative to the ray's largest reference magnitude (one scale for the ray's six outputs,
# one for its gradients).  The yardstick is the SAME restatement evaluated in float32 by torch on the CPU (double sum, cumprod, autograd), which
# is not the code under test: its largest gap to the float64 evaluation over every case below (restatement_gaps() reproduces it) is
#   forward 2.1e-4, gradients 6.9e-4      (both on the S = 256 case; the faint ray sets them: alpha = 1 - exp(-delta sigma) cancels in float32
#                                          for delta sigma ~ 1e-5, in the restatement as in the kernels, which take alpha as the composite does)
# The kernels get four times that gap, because their summation order (wave scans) and exponential differ from torch's.
# (Measured on an MI355X over all cases: forward 1.6e-6 — the kernels form alpha as -expm1(-delta sigma) — and 1.9e-4 on the gradients.)
GAP_F32_FWD = 2.1e-4
GAP_F32_BWD = 6.9e-4
BOUND_FWD = 4 * GAP_F32_FWD
BOUND_BWD = 4 * GAP_F32_BWD

SHAPES = [(3, 2), (32, 32), (33, 32), (128, 128)]          # S = 5 partial chunk, 64 one chunk, 65 carry across chunks, 256 the maximum
RAYS = [1, 5]                                               # not multiples of the kernels' four rays per workgroup
THR = 0.5


def make_inputs(N, T, t, seed=0):
    """float32 CPU inputs: sorted z with a duplicate, sigma log-uniform over six decades, rgbc in (0, 1).  With N = 5: ray 1 has sigma = 0,
    ray 2 an opaque first sample (the transmittance underflows behind it), ray 3 misses the box (far == near), ray 4 weighs less than the
    entropy's min_opacity."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * (T + t) + N)
    S = T + t
    nears = 0.2 + torch.rand(N, generator=g)
    fars = nears + 1.0 + torch.rand(N, generator=g)
    L = (fars - nears)[:, None]
    z = (nears[:, None] + L * torch.rand(N, S, generator=g)).sort(1).values
    sigma = 10 ** (torch.rand(N, S, generator=g) * 6 - 3)
    rgbc = torch.rand(N, S, 4, generator=g) * 0.98 + 0.01
    # every other sample sits in the soft mask's transition zone (sigmoid((conf - 0.5) * 100) saturates in float32 beyond |conf - 0.5| = 0.17)
    rgbc[:, ::2, 3] = (0.5 + 0.03 * torch.randn(N, (S + 1) // 2, generator=g)).clamp(0.01, 0.99)
    if N >= 5:
        sigma[1] = 0
        z[2] = torch.cat([nears[2:3] + 0.01 * L[2], (nears[2] + 0.1 * L[2] + 0.9 * L[2] * torch.rand(S - 1, generator=g)).sort().values])
        sigma[2, 0] = 1e6
        rgbc[2, 0, 3] = 0.9                  # inside the edit region: detach_bg must not remove the one sample that carries the ray's gradient
        fars[3] = nears[3]
        z[3] = nears[3]
        sigma[4] = 10 ** (torch.rand(S, generator=g) - 3)
    z[:, 2] = z[:, 1]                        # a repeated sample: delta = 0
    z = z.clamp(nears[:, None], fars[:, None])
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    g_reg = torch.randn(3, N, 2, generator=g)
    return sigma.contiguous(), rgbc.contiguous(), z.contiguous(), nears, fars, g_reg


@functools.lru_cache(maxsize=None)
def reference(N, T, t, soft, detach_bg, dtype=torch.float64):
    sigma, rgbc, z, nears, fars, g_reg = make_inputs(N, T, t)
    return rs.regularizers_with_grads(sigma, rgbc, z, nears, fars, T, soft, THR, g_reg, detach_bg, dtype=dtype)


def ray_gap(got, ref, name):
    """got, ref [N, ...]: largest |got - ref| of a ray over the ray's largest |ref|; a ray whose reference is all zero must be all zero, and
    nothing may be NaN"""
    got, ref = got.detach().cpu().double().reshape(ref.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    assert not torch.isnan(got).any(), f"{name}: NaN"
    scale = ref.abs().amax(1)
    zero = scale == 0
    if bool(zero.any()):
        assert float(got[zero].abs().max()) == 0.0, f"{name}: a ray that must be exactly zero is not"
    err = (got - ref).abs().amax(1)
    return float((err[~zero] / scale[~zero]).max()) if bool((~zero).any()) else 0.0


def restatement_gaps():
    """the float32 restatement against the float64 one on every case of test_forward_backward_against_float64: (forward, backward) maxima"""
    fwd = bwd = 0.0
    for N in RAYS:
        for T, t in SHAPES:
            for soft in (True, False):
                for detach_bg in (False, True):
                    o64, s64, c64 = reference(N, T, t, soft, detach_bg)
                    o32, s32, c32 = reference(N, T, t, soft, detach_bg, torch.float32)
                    f = ray_gap(o32.permute(1, 0, 2), o64.permute(1, 0, 2), "out")
                    b = ray_gap(torch.cat([s32, c32[..., 3]], 1), torch.cat([s64, c64[..., 3]], 1), "gradients")
                    print(f"N {N} S {T + t} soft {soft} detach_bg {detach_bg}: float32 restatement gap forward {f:.2e} backward {b:.2e}")
                    fwd, bwd = max(fwd, f), max(bwd, b)
    return fwd, bwd


def _run(N, T, t, soft, detach_bg, variants=7, g_reg=None, src=None, min_opacity=0.1, sigma=None, rgbc=None):
    from customnerf_amd.nerf import render_ops
    s0, c0, z, nears, fars, g0 = make_inputs(N, T, t)
    s = (s0 if sigma is None else sigma).cuda().reshape(-1).requires_grad_(True)
    c = (c0 if rgbc is None else rgbc).cuda().reshape(-1, 4).requires_grad_(True)
    out = render_ops.ray_regularizers(s, c, z.cuda(), src, nears.cuda(), fars.cuda(), T, soft, THR, detach_bg, variants, min_opacity)
    out.backward((g0 if g_reg is None else g_reg).cuda())
    return out.detach(), s.grad, c.grad


@pytest.mark.gpu
@pytest.mark.parametrize("detach_bg", [False, True])
@pytest.mark.parametrize("soft", [True, False])
@pytest.mark.parametrize("T, t", SHAPES)
@pytest.mark.parametrize("N", RAYS)
def test_forward_backward_against_float64(N, T, t, soft, detach_bg):
    ref_out, ref_gs, ref_gc = reference(N, T, t, soft, detach_bg)
    out, gs, gc = _run(N, T, t, soft, detach_bg)
    assert out.shape == (3, N, 2)
    f = ray_gap(out.permute(1, 0, 2), ref_out.permute(1, 0, 2), "out")
    if soft:
        assert float(gc[..., :3].abs().max()) == 0.0                      # no gradient to rgb
        g_conf = gc.view(N, T + t, 4)[..., 3]
        assert float(g_conf.abs().max()) > 0
    else:
        assert gc is None and float(ref_gc.abs().max()) == 0.0            # hard mask: nothing depends on the confidence
        g_conf = torch.zeros(N, T + t, device="cuda")
    # one scale per ray: the largest reference gradient of the ray, density or confidence
    b = ray_gap(torch.cat([gs.view(N, T + t), g_conf], 1), torch.cat([ref_gs, ref_gc[..., 3]], 1), "gradients")
    print(f"N {N} S {T + t} soft {soft} detach_bg {detach_bg}: forward gap {f:.2e} (bound {BOUND_FWD:.1e}), backward gap {b:.2e} (bound {BOUND_BWD:.1e})")
    assert float(ref_gs.abs().max()) > 0 and float(ref_out.abs().max()) > 0
    assert f <= BOUND_FWD, (f, BOUND_FWD)
    assert b <= BOUND_BWD, (b, BOUND_BWD)
    if N == 5:
        assert float(out[:, 3].abs().max()) == 0.0 and float(gs.view(N, -1)[3].abs().max()) == 0.0        # far == near
        assert float(out[:, 4, 1].abs().max()) == 0.0 and float(out[0, 0, 1]) > 0                          # the entropy gate


@pytest.mark.gpu
@pytest.mark.parametrize("T, t", SHAPES)
def test_indexed_equals_plain_bit_for_bit(T, t):
    N, S = 5, T + t
    sigma, rgbc, z, nears, fars, g_reg = make_inputs(N, T, t)
    g = torch.Generator().manual_seed(7)
    perm = torch.stack([torch.randperm(S, generator=g) for _ in range(N)])
    src = (torch.arange(N)[:, None] * S + perm).to(torch.int32)              # row of every sorted position
    sig_l, rgbc_l = torch.empty(N * S), torch.empty(N * S, 4)
    sig_l[src.long().reshape(-1)] = sigma.reshape(-1)
    rgbc_l[src.long().reshape(-1)] = rgbc.reshape(-1, 4)
    for soft in (True, False):
        out, gs, gc = _run(N, T, t, soft, True)
        out_i, gs_i, gc_i = _run(N, T, t, soft, True, src=src.cuda(), sigma=sig_l, rgbc=rgbc_l)
        assert torch.equal(out, out_i)
        assert torch.equal(gs, gs_i[src.long().reshape(-1).cuda()])
        if soft:
            assert torch.equal(gc, gc_i[src.long().reshape(-1).cuda()]) and float(gc[..., 3].abs().max()) > 0


@pytest.mark.gpu
def test_reproducible_and_variant_selection():
    N, T, t = 5, 33, 32
    _, _, _, _, _, g_reg = make_inputs(N, T, t)
    a, b = _run(N, T, t, True, False), _run(N, T, t, True, False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                               # no atomics: the same bits twice
    out1, gs1, gc1 = _run(N, T, t, True, False, variants=1)
    assert torch.equal(out1[0], a[0][0]) and float(out1[1:].abs().max()) == 0.0 and gc1 is None
    out5, gs5, gc5 = _run(N, T, t, True, False, variants=5)
    assert torch.equal(out5[0], a[0][0]) and torch.equal(out5[2], a[0][2]) and float(out5[1].abs().max()) == 0.0
    # a variant that was not computed gets no gradient whatever arrives for its rows, and one with a zero incoming gradient adds exactly nothing
    g0 = g_reg.clone()
    g0[1:] = 0
    _, gs0, gc0 = _run(N, T, t, True, False, g_reg=g0)
    assert torch.equal(gs0, gs1) and float(gc0.abs().max()) == 0.0
    g02 = g_reg.clone()
    g02[1] = 0
    _, gs02, gc02 = _run(N, T, t, True, False, g_reg=g02)
    assert torch.equal(gs02, gs5) and torch.equal(gc02, gc5)
    assert not torch.equal(gs5, gs1) and not torch.equal(a[1], gs5)


# ------------------------------------------------------------------------------------------------ renderer
def _tiny_model(fp16, hw=8, **optkw):
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider_utils import generate_rays
    tcnn.set_default_dtype(torch.float16 if fp16 else torch.float32)
    torch.manual_seed(0)
    opt = sc.make_opt(fp16=fp16, num_levels=8, log2_hashmap_size=15, desired_resolution=256, num_steps=32, upsample_steps=32, lr=5e-3, iters=200, **optkw)
    model = NeRFNetwork(opt).cuda().train()
    with torch.no_grad():
        model.pos_en.embeddings.uniform_(-0.5, 0.5)
    H = W = hw
    c2w = torch.from_numpy(sc.poses(4)).cuda()
    o, d = generate_rays(c2w, *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
    o, d = o.view(4, 1, H * W, 3), d.view(4, 1, H * W, 3)
    g = torch.Generator(device="cuda").manual_seed(3)
    draws = dict(z=torch.rand(H * W, 32, device="cuda", generator=g), u=torch.rand(H * W, 32, device="cuda", generator=g))
    return opt, model, o, d, draws, (H, W)


NEW_KEYS = ("distortion", "ray_entropy")


@pytest.mark.gpu
@pytest.mark.parametrize("split", [True, False])
def test_renderer_adds_the_keys_and_their_gradient_reaches_the_field(split):
    from customnerf_amd.nerf import render_ops
    opt, model, o, d, draws, (H, W) = _tiny_model(False, split_eval=split)
    kw = dict(num_steps=32, upsample_steps=32, perturb=True, _draws=draws)
    plain = model.run(o[0], d[0], **kw)
    for r in (plain, plain['fg'], plain['bg']):
        assert not any(k in r for k in NEW_KEYS)
    seen = {}
    orig = render_ops.ray_regularizers

    def tap(*a, **k):
        seen['args'], seen['kw'] = a, k
        return orig(*a, **k)
    render_ops.ray_regularizers = tap
    try:
        res = model.run(o[0], d[0], ray_reg=True, **kw)
    finally:
        render_ops.ray_regularizers = orig
    assert (seen['args'][3] is not None) == split                           # the split sample list goes through its index
    # the values of ray_regularizers on the sorted sigma / rgbc / z_vals that the result dict exposes
    N, S = H * W, 64
    sig = res['sigma'].detach().reshape(N * S)
    conf = seen['args'][1].detach().reshape(-1, 4)[:, 3]                     # (the dict exposes the confidence only through edit_mask)
    if split:
        conf = conf[seen['args'][3].long().reshape(-1)]                       # sample-list order -> sorted order
    rgbc = torch.cat([res['rgbs'].detach().reshape(N * S, 3), conf.reshape(N * S, 1)], -1)
    nears, fars = seen['args'][4], seen['args'][5]
    want = orig(sig, rgbc, res['z_vals'], None, nears, fars, 32, bool(opt.soft_mask), float(opt.conf_thr), bool(opt.detach_bg), 7, 0.1)
    for v, r in enumerate((res, res['fg'], res['bg'])):
        assert r['distortion'].shape == (1, N) and r['ray_entropy'].shape == (1, N)
        assert torch.equal(r['distortion'].reshape(-1), want[v, :, 0]) and torch.equal(r['ray_entropy'].reshape(-1), want[v, :, 1])
    assert float(res['distortion'].detach().max()) > 0 and float(res['ray_entropy'].detach().max()) > 0
    for p in model.parameters():
        p.grad = None
    res['distortion'].mean().backward()
    for name in ("pos_en.embeddings", "network.params", "density_network.params"):
        gr = dict(model.named_parameters())[name].grad
        assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().max()) > 0, name


@pytest.mark.gpu
def test_early_termination_flags_are_ignored_when_the_regulariser_adds_its_gradient():
    """loss = 0 * composite + distortion: the compositing backward reports every tile dead (its gradient is all zero) while the regulariser's
    gradient is live on the same sigma.  The field backward must not trust the flags: the parameter gradients are non-zero and bit-identical
    to the step without early termination (the composite adds exact zeros in both)."""
    from customnerf_amd import field as fld
    from customnerf_amd.trainer import ReconTrainer
    # (64 x 64 rays: from 2^20 (sample, level) pairs on the grid scatter takes its path without float atomics, whose sums are reproducible)
    opt, model, o, d, draws, _ = _tiny_model(True, hw=64)
    tr = ReconTrainer(model, opt, fp16=True)
    assert model._fused_cfg() and model._half()
    used, grads = [], {}
    orig_b = fld.FieldFunction.backward

    def spy(ctx, g_sigma, g_rgbc):
        flags = getattr(g_sigma, '_cnerf_tile_live', None)
        ok = flags is not None and g_sigma.data_ptr() == flags[1] and g_sigma._version == flags[2] and g_rgbc.data_ptr() == flags[3] and g_rgbc._version == flags[4]
        used.append((flags is not None, ok))
        return orig_b(ctx, g_sigma, g_rgbc)
    fld.FieldFunction.backward = staticmethod(spy)
    try:
        for et, reg in ((True, True), (False, True), (True, False)):
            model.opt.early_termination = et
            for p in model.parameters():
                p.grad.zero_()
            with torch.autocast('cuda', dtype=torch.float16):
                res = model.render(o[1], d[1], staged=False, perturb=True, force_all_rays=True, _draws=draws, num_steps=32, upsample_steps=32, ray_reg=True)
                loss = 0 * res['_out_ray'].sum() + (res['distortion'].mean() if reg else 0.0)
            tr.scaler.backward(loss)
            grads[(et, reg)] = [p.grad.detach().clone() for p in model.parameters()]
    finally:
        fld.FieldFunction.backward = orig_b
        model.opt.early_termination = True
    (had1, ok1), (had2, _), (had3, ok3) = used
    assert not ok1 and not had2                                 # accumulated into: whatever arrived no longer describes the tensors
    assert had3 and ok3                                         # the composite alone: the flags arrive intact (and every tile is dead)
    names = [n for n, _ in model.named_parameters()]
    for name, a, b, c in zip(names, grads[(True, True)], grads[(False, True)], grads[(True, False)]):
        # (the colour network sees nothing of the `all` variant's distortion: no gradient to rgb, and the confidence enters the other variants only)
        assert torch.isfinite(a).all() and (float(a.abs().max()) > 0) == (not name.startswith("rgb_network")), name
        assert torch.equal(a, b), name
        assert float(c.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ trainers
@pytest.mark.gpu
def test_recon_trainer_adds_the_weighted_mean_to_the_loss():
    from customnerf_amd import scene as sc
    from customnerf_amd.trainer import ReconTrainer
    lam = 0.05
    opt, model, o, d, draws, (H, W) = _tiny_model(True)
    rgb, mask = sc.targets(4, H, W)
    rgb, mask = rgb.cuda(), mask.cuda()
    models = [model, copy.deepcopy(model), copy.deepcopy(model)]
    opts = [argparse.Namespace(**dict(vars(opt), lambda_distortion=l)) for l in (lam, 0.0, 0.0)]
    for m, op in zip(models, opts):
        m.opt = op
    trs = [ReconTrainer(m, op, fp16=True) for m, op in zip(models, opts)]
    before = [p.detach().clone() for p in model.parameters()]
    kw = dict(num_steps=32, upsample_steps=32, _draws=draws)
    loss_a, out_a = trs[0].train_step(o[0], d[0], rgb[0], mask[0], **kw)
    loss_b, out_b = trs[1].train_step(o[0], d[0], rgb[0], mask[0], ray_reg=True, **kw)      # lambda = 0: the recon term, and the regulariser beside it
    loss_c, out_c = trs[2].train_step(o[0], d[0], rgb[0], mask[0], **kw)
    assert 'distortion' in out_a and 'distortion' in out_b
    assert not any(k in out_c for k in NEW_KEYS) and 'fg' not in out_c
    assert torch.equal(out_a['distortion'], out_b['distortion']) and float(loss_b) == float(loss_c)
    assert np.isfinite(float(loss_a))
    reg = float(out_b['distortion'].float().mean())
    assert reg > 0
    np.testing.assert_allclose(float(loss_a), float(loss_b) + lam * reg, rtol=1e-6)
    moved = differs = 0.0
    for p0, pa, pb, pc in zip(before, models[0].parameters(), models[1].parameters(), models[2].parameters()):
        assert torch.isfinite(pa).all()
        moved = max(moved, float((pa - p0).abs().max()))
        differs = max(differs, float((pa - pb).abs().max()))
    assert moved > 0 and differs > 0


@pytest.mark.gpu
@pytest.mark.parametrize("region", ["all", "fg"])
def test_edit_trainer_adds_the_terms_on_the_named_region(region):
    from customnerf_amd import scene as sc
    from customnerf_amd.sd.editing import EditTrainer
    lam_d, lam_h = 0.05, 0.01
    opt, model, o, d, _, (H, W) = _tiny_model(True, cfg=7.5, log_loss_item=False, keep_bg=10.0, lambda_sd=0.0)
    pre = copy.deepcopy(model).eval()
    guide = argparse.Namespace(set_system=lambda system: None)             # lambda_sd = 0: the step never asks the guidance for anything
    rgb, mask = sc.targets(4, H, W)
    data = (rgb[0].cuda(), mask[0].cuda(), o[0], d[0], H, W, "v0")
    m_reg, m_ref = model, copy.deepcopy(model)
    m_reg.opt = argparse.Namespace(**dict(vars(opt), lambda_distortion=lam_d, lambda_ray_entropy=lam_h, ray_reg_region=region))
    m_ref.opt = argparse.Namespace(**dict(vars(opt), ray_reg=True))         # lambda = 0, but the renderer is asked for the two maps
    tr_ref = EditTrainer(m_ref, pre, guide, m_ref.opt, None, None)
    tr_reg = EditTrainer(m_reg, copy.deepcopy(pre), guide, m_reg.opt, None, None)
    seen = []
    orig = m_ref.render
    m_ref.render = lambda *a, **k: seen.append(orig(*a, **k)) or seen[-1]
    torch.manual_seed(11)
    loss_ref, ld_ref = tr_ref.train_step(data)
    torch.manual_seed(11)
    loss_reg, ld_reg = tr_reg.train_step(data)
    assert set(ld_ref) == {"loss_bg"} and set(ld_reg) == {"loss_bg", "loss_distortion", "loss_ray_entropy"}
    src = seen[0] if region == 'all' else seen[0]['fg']
    want_d, want_h = lam_d * float(src['distortion'].float().mean()), lam_h * float(src['ray_entropy'].float().mean())
    assert want_d > 0 and want_h >= 0
    np.testing.assert_allclose(float(ld_reg['loss_distortion']), want_d, rtol=1e-6)
    np.testing.assert_allclose(float(ld_reg['loss_ray_entropy']), want_h, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(float(loss_reg), float(loss_ref) + want_d + want_h, rtol=2e-6)
    assert np.isfinite(float(loss_reg))
    differs = max(float((a - b).abs().max()) for a, b in zip(m_reg.parameters(), m_ref.parameters()))
    assert differs > 0 and all(torch.isfinite(p).all() for p in m_reg.parameters())
    # the multi-view step: the mean over the views of the single-view terms
    torch.manual_seed(12)
    _, ld2 = tr_reg.train_step_multi([data, data])
    assert {"loss_distortion", "loss_ray_entropy"} <= set(ld2) and np.isfinite(float(ld2['loss_distortion'])) and float(ld2['loss_distortion']) > 0
