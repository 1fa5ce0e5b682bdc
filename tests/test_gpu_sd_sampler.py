"""GPU: DDIM sampling and the SDS preview.  cnerf_sd_ddim_step against the float64 formula, StableDiffusion.produce_latents against the
DDIM loop of tests/vae_decoder_restatement.py (closed-form epsilon, then the real small UNet against oracle/sd_oracle.py),
embeds_to_img, and EditTrainer.guidance_preview, which must leave a training run bit for bit where it was."""
import copy
import math
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import vae_decoder_restatement as R  # noqa: E402
from oracle import sd_oracle as so  # noqa: E402

# produce_latents with the real small UNet (float16 activations, 3 steps) against the loop over the float32 torch oracle, L2-relative on the
# final latents.  Measured on MI355X: 3.8e-3 (one UNet call alone is 1.4e-3 .. 1.7e-3, tests/test_gpu_sd_nets.py; three of them feed each
# other); bound = 3 x
SAMPLE_L2_REL = 1.15e-2
# the decoder's bound of tests/test_gpu_sd_decode.py (max-relative, float16 decoder against its float32 restatement)
DEC_MAX_REL = 3.8e-3


def half_sd(sd):
    return {k: (v.half().float() if v.dim() > 1 else v) for k, v in sd.items()}


def _opt(**kw):
    return types.SimpleNamespace(**dict(dict(cfg=7.5, lambda_sd=0.01, max_ratio=0.98, stage_time=False, iters=10, log_loss_item=False), **kw))


def _guide(use_graph=True, seed=0, **kw):
    from customnerf_amd.sd import arch
    from customnerf_amd.sd.guidance import StableDiffusion
    return StableDiffusion("cuda", "1.5", _opt(), unet_cfg=arch.UNET_TINY, vae_cfg=arch.VAE_TINY, seed=seed, use_graph=use_graph, **kw)


def _nchw(e):
    return e.permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("mode", ["cfg", "sds"])
@pytest.mark.parametrize("pairs", [1, 3])
def test_ddim_step_kernel(mode, pairs):
    """float32 arithmetic on O(1) values against float64 on the same half eps: latents and x0 at rtol 1e-5 / atol 1e-6, the half UNet-input
    copy exactly .half() of the float32 latents in both CFG slots with zero padding; every output may be left out on its own."""
    from customnerf_amd.sd import ops
    h, w, ld = 5, 7, 8                                                          # 35 pixels: odd, no multiple of the wave
    g = torch.Generator().manual_seed(11 + pairs)
    eps = torch.randn(2 * pairs, h, w, ld, generator=g).half()                  # columns 4..7: garbage the kernel must not read into the result
    x = torch.randn(pairs, 4, h, w, generator=g)
    ab_t, ab_p, gs = 0.4, 0.55, 7.5
    m = ops.DDIM_SDS if mode == "sds" else ops.DDIM_CFG
    lat_o, x0_o, u_o = torch.empty(pairs, 4, h, w).cuda(), torch.empty(pairs, 4, h, w).cuda(), torch.full((2 * pairs, h, w, 8), 7.0, dtype=torch.float16).cuda()
    ops.ddim_step(eps.cuda(), x.cuda(), ab_t, ab_p, gs, m, latents_out=lat_o, x0_out=x0_o, unet_in=u_o)
    # float64 on the values the kernel receives: float32 alpha_bars and guidance, half eps
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    e = _nchw(eps[..., :4].double())
    e_u, e_t = e[0::2], e[1::2]
    ref_prev, ref_x0 = R.ddim_step(x.double(), e_u, e_t, f32(ab_t), f32(ab_p), f32(gs), sds=(mode == "sds"))
    torch.testing.assert_close(lat_o.cpu().double(), ref_prev, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(x0_o.cpu().double(), ref_x0, rtol=1e-5, atol=1e-6)
    u = u_o.cpu()
    want = lat_o.cpu().half().permute(0, 2, 3, 1)                               # [pairs, h, w, 4]
    assert torch.equal(u[0::2, ..., :4], want) and torch.equal(u[1::2, ..., :4], want) and not u[..., 4:].any()
    # the two combinations differ, and so do the two slots: a swapped pair or a wrong mode cannot pass
    other = R.ddim_step(x.double(), e_u, e_t, f32(ab_t), f32(ab_p), f32(gs), sds=(mode != "sds"))[1]
    swapped = R.ddim_step(x.double(), e_t, e_u, f32(ab_t), f32(ab_p), f32(gs), sds=(mode == "sds"))[1]
    assert float((other - ref_x0).abs().max()) > 0.1 and float((swapped - ref_x0).abs().max()) > 0.1
    # each output alone gives the same bits; x_prev may overwrite x
    only = torch.empty_like(lat_o)
    ops.ddim_step(eps.cuda(), x.cuda(), ab_t, ab_p, gs, m, latents_out=only)
    assert torch.equal(only, lat_o)
    only = torch.empty_like(x0_o)
    ops.ddim_step(eps.cuda(), x.cuda(), ab_t, ab_p, gs, m, x0_out=only)
    assert torch.equal(only, x0_o)
    only = torch.empty_like(u_o)
    ops.ddim_step(eps.cuda(), x.cuda(), ab_t, ab_p, gs, m, unet_in=only)
    assert torch.equal(only, u_o)
    inplace = x.cuda()
    ops.ddim_step(eps.cuda(), inplace, ab_t, ab_p, gs, m, latents_out=inplace)
    assert torch.equal(inplace, lat_o)
    # a contiguous eps without padding (ld = 4: what the UNet returns)
    lat4 = torch.empty_like(lat_o)
    ops.ddim_step(eps[..., :4].contiguous().cuda(), x.cuda(), ab_t, ab_p, gs, m, latents_out=lat4)
    assert torch.equal(lat4, lat_o)


# ------------------------------------------------------------------------------------------------ the loop, closed-form epsilon
@pytest.mark.parametrize("gs", [0.0, 7.5])
def test_produce_latents_with_closed_form_epsilon(gs):
    """eps_pred replaced by the exact noise of a fixed x0* (text half) and a different one (uncond half), returned as [2B, h, w, 8] half:
    latents and every step's x0 against the restatement loop fed the same half eps.  Tolerance: rtol 1e-4 per element, plus 1e-6 of the
    tensor's largest value for the elements that cancel to about zero (float32 round-off does not shrink with them)."""
    guide = _guide()
    a = guide.alphas_host
    g = torch.Generator().manual_seed(5)
    B, h, w, n = 2, 16, 16, 5
    x0_star = torch.randn(B, 4, h, w, generator=g)
    start = torch.randn(B, 4, h, w, generator=g)
    star = x0_star.permute(0, 2, 3, 1).cuda()
    fed, seen_t = [], []

    def eps_pred(unet_in, t, text_embeddings):
        assert unet_in.shape == (2 * B, h, w, 8) and unet_in.dtype == torch.float16
        assert torch.equal(unet_in[0::2], unet_in[1::2]) and not unet_in[..., 4:].any()          # the CFG pair, zero padding
        if not fed:
            assert torch.equal(unet_in[0::2, ..., :4], start.half().permute(0, 2, 3, 1).cuda())  # the first input: the initial noise itself
        ab = float(a[t])
        e_t = (unet_in[1::2, ..., :4].float() - math.sqrt(ab) * star) / math.sqrt(1 - ab)
        e_u = 0.5 * e_t + 0.1
        out = torch.full((2 * B, h, w, 8), 3.0, dtype=torch.float16, device="cuda")
        out[0::2, ..., :4], out[1::2, ..., :4] = e_u.half(), e_t.half()
        fed.append(out.cpu())
        seen_t.append(t)
        return out

    guide.eps_pred = eps_pred
    start_dev = start.cuda()
    lat, x0s = guide.produce_latents(guide.synthetic_text_embeds(0), 128, 128, num_inference_steps=n, guidance_scale=gs, latents=start_dev, return_x0=True)
    assert seen_t == [801, 601, 401, 201, 1] and lat.shape == (B, 4, h, w) and x0s.shape == (n, B, 4, h, w)
    it = iter(fed)

    def eps_fn(x, t):
        e = _nchw(next(it)[..., :4].float())
        return e[0::2], e[1::2]

    ref, ref_x0s = R.ddim_loop(eps_fn, start, a, n, gs)

    def close(got, want):
        got, want = got.cpu(), want
        return bool(((got - want).abs() <= 1e-4 * want.abs() + 1e-6 * want.abs().max()).all())

    assert close(lat, ref)
    for i in range(n):
        assert close(x0s[i], ref_x0s[i]), i
    if gs == 0.0:
        # no guidance: the prediction is the uncond half's alone (e_u = 0.5 e_t + 0.1, so x0 is NOT x0*) ...
        assert float((x0s[0].cpu() - x0_star).abs().max()) > 0.1
    assert torch.equal(start_dev.cpu(), start) and lat.data_ptr() != start_dev.data_ptr()      # the caller's noise is left alone


def test_guidance_scale_enters_only_through_the_pair():
    """same run under g = 0 and g = 1: g = 1 is the text half alone, whose eps is exact for x0* -> every x0 is x0*; g = 0 is the uncond half alone"""
    guide = _guide()
    a = guide.alphas_host
    g = torch.Generator().manual_seed(6)
    x0_star, start = torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g)
    star = x0_star.permute(0, 2, 3, 1).cuda()

    def eps_pred(unet_in, t, text_embeddings):
        ab = float(a[t])
        e_t = (unet_in[1::2, ..., :4].float() - math.sqrt(ab) * star) / math.sqrt(1 - ab)
        out = torch.zeros(2, 16, 16, 8, dtype=torch.float16, device="cuda")
        out[0::2, ..., :4], out[1::2, ..., :4] = (0.5 * e_t + 0.1).half(), e_t.half()
        return out

    guide.eps_pred = eps_pred
    text = guide.synthetic_text_embeds(0)
    _, x0_1 = guide.produce_latents(text, 128, 128, num_inference_steps=5, guidance_scale=1.0, latents=start.cuda(), return_x0=True)
    _, x0_0 = guide.produce_latents(text, 128, 128, num_inference_steps=5, guidance_scale=0.0, latents=start.cuda(), return_x0=True)
    # half eps and half UNet input: x0 = x0* up to 2^-11 relative round-off of eps and x, divided by sqrt(alpha_bar) >= 0.2 from step 2 on
    assert float((x0_1[1:].cpu() - x0_star).abs().max()) < 0.05
    assert float((x0_0[1:].cpu() - x0_star).abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------ the loop, real UNet
def test_produce_latents_real_unet_graph_eager_and_oracle():
    from customnerf_amd.sd import arch
    g = torch.Generator().manual_seed(8)
    start = torch.randn(1, 4, 16, 16, generator=g)
    graph, eager = _guide(use_graph=True, seed=2), _guide(use_graph=False, seed=2)
    text = graph.synthetic_text_embeds(3).half().float()
    lat_g = graph.produce_latents(text, 128, 128, num_inference_steps=3, guidance_scale=7.5, latents=start.cuda())
    lat_g2 = graph.produce_latents(text, 128, 128, num_inference_steps=3, guidance_scale=7.5, latents=start.cuda())      # replay
    lat_e = eager.produce_latents(text, 128, 128, num_inference_steps=3, guidance_scale=7.5, latents=start.cuda())
    assert torch.equal(lat_g, lat_e) and torch.equal(lat_g2, lat_g)
    usd = half_sd(arch.random_state_dict(arch.unet_params(arch.UNET_TINY), 2 + 1))
    ts = []

    def eps_fn(x, t):
        ts.append(t)
        with torch.no_grad():
            e = so.unet_forward(usd, arch.UNET_TINY, torch.cat([x, x]), torch.full((2,), float(t)), text.cpu())
        return e[0:1], e[1:2]

    ref, _ = R.ddim_loop(eps_fn, start, graph.alphas_host, 3, 7.5)
    assert ts == [667, 334, 1]
    err = float((lat_g.cpu() - ref).norm() / ref.norm())
    print(f"[produce_latents tiny, 3 steps] L2 rel vs the oracle loop {err:.3e}")
    assert err < SAMPLE_L2_REL, err


def test_embeds_to_img_shapes_reproducibility_and_argument_checks():
    guide = _guide()
    text = guide.synthetic_text_embeds(0)
    img = guide.embeds_to_img(text, 128, 128, num_inference_steps=2, generator=torch.Generator().manual_seed(5), batch_size=2)
    assert img.shape == (2, 128, 128, 3) and img.dtype == torch.uint8 and img.is_cuda
    again = guide.embeds_to_img(text, 128, 128, num_inference_steps=2, generator=torch.Generator().manual_seed(5), batch_size=2)
    assert torch.equal(img, again) and not torch.equal(img[0], img[1])
    other = guide.embeds_to_img(text, 128, 128, num_inference_steps=2, generator=torch.Generator().manual_seed(6), batch_size=2)
    assert not torch.equal(other, img)
    before = guide._gen.get_state()
    with pytest.raises(ValueError):
        guide.produce_latents(text, height=100, width=128)
    with pytest.raises(ValueError):
        guide.produce_latents(text, height=128, width=128, latents=torch.zeros(1, 4, 8, 8))
    with pytest.raises(NotImplementedError):
        guide.prompt_to_img("a corgi")
    assert torch.equal(guide._gen.get_state(), before)                          # the training timestep stream is not drawn from
    assert len(guide._ctx_cache) == 1


# ------------------------------------------------------------------------------------------------ the preview inside a training run
def _trainer(res=128):
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider_utils import generate_rays
    from customnerf_amd.sd import arch
    from customnerf_amd.sd.guidance import StableDiffusion
    from customnerf_amd.sd.editing import EditTrainer
    tcnn.set_default_dtype(torch.float16)
    torch.manual_seed(0)
    opt = sc.make_opt(fp16=True, num_levels=8, num_steps=16, upsample_steps=16, cfg=7.5, log_loss_item=False, keep_bg=1000.0, lambda_sd=0.01,
                      sds_resolution=res)
    model = NeRFNetwork(opt).cuda()
    with torch.no_grad():
        model.pos_en.embeddings.uniform_(-0.5, 0.5)
    pre = copy.deepcopy(model).eval()
    guide = StableDiffusion("cuda", "1.5", opt, unet_cfg=arch.UNET_TINY, vae_cfg=arch.VAE_TINY, seed=0)
    H = W = res
    c2w = torch.from_numpy(sc.poses(2)).cuda()
    o, d = generate_rays(c2w, *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
    o, d = o.view(2, 1, H * W, 3), d.view(2, 1, H * W, 3)
    rgb, mask = sc.targets(2, H, W)
    tr = EditTrainer(model, pre, guide, opt, guide.synthetic_text_embeds(0), guide.synthetic_text_embeds(1))
    return tr, model, lambda v: (rgb[v].cuda(), mask[v].cuda(), o[v], d[v], H, W, f"v{v}")


def test_guidance_preview_leaves_the_training_run_alone(tmp_path):
    from customnerf_amd.sd import arch, ops
    res = 128
    # run A: four steps
    tr, model, data = _trainer(res)
    losses_a = [tr.train_step(data(i % 2)) for i in range(4)]
    params_a = {n: p.detach().clone() for n, p in model.named_parameters()}
    # run B: two steps, a preview (and this test's own look at what it showed), two more
    tr, model, data = _trainer(res)
    losses_b = [tr.train_step(data(i % 2)) for i in range(2)]
    png = tmp_path / "preview.png"
    strip = tr.guidance_preview(data(0), path=str(png), seed=0)
    assert strip.shape == (res, 3 * res, 3) and strip.dtype == torch.uint8
    assert png.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    assert torch.equal(strip, tr.guidance_preview(data(0), seed=0)) and tr.global_step == 2

    # the x0 panel: the restatement's one-step estimate from the same render, draws and UNet prediction, decoded by the restatement
    guide = tr.guidance
    rays_o, rays_d = data(0)[2], data(0)[3]
    model.eval()                                                                # the deterministic render: no importance-sampling draws
    img = tr._render_eval(model, rays_o, rays_d)['image'].reshape(1, res, res, 3).permute(0, 3, 1, 2).float().contiguous()
    model.train()
    assert torch.equal(strip[:, :res], (img[0].permute(1, 2, 0).clamp(0, 1) * 255.0).round().to(torch.uint8))
    gen = torch.Generator().manual_seed(0)
    sample_noise, noise = torch.randn(2, 1, 4, res // 8, res // 8, generator=gen).unbind(0)
    t = (guide.min_step + guide.max_step) // 2
    assert t == 500
    ab = float(guide.alphas_host[t])
    with torch.no_grad():
        lat = guide.encode_imgs(img, sample_noise=sample_noise.cuda(), resize=(res, res))
        eps = guide.eps_pred(ops.add_noise(lat, noise.cuda(), ab), t, tr.text_z).float().cpu()
    e = _nchw(eps)
    noisy = math.sqrt(ab) * lat.cpu() + math.sqrt(1 - ab) * noise
    _, x0 = R.ddim_step(noisy, e[0:1], e[1:2], ab, ab, 7.5, sds=True)
    dec_sd = half_sd(arch.random_state_dict(arch.vae_decoder_params(arch.VAE_TINY), 0 + 3))
    with torch.no_grad():
        raw = R.decode(dec_sd, arch.VAE_TINY, torch.cat([noisy, x0]))
    ref = (raw / 2 + 0.5).clamp(0, 1)
    for k, name in ((0, "noisy"), (1, "x0")):
        tol = 0.5 * DEC_MAX_REL * float(raw[k].abs().max()) + 0.5 / 255 + 1e-6  # the decoder's bound on the raw output, halved by x / 2 + 0.5, + the uint8 rounding
        panel = strip[:, (k + 1) * res:(k + 2) * res].float().cpu() / 255
        err = float((panel - ref[k].permute(1, 2, 0)).abs().max())
        print(f"[guidance_preview] {name} panel max |diff| {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, (name, err, tol)
    assert not torch.equal(strip[:, res:2 * res], strip[:, 2 * res:])
    # preview's other mode: the estimate under plain classifier-free guidance
    _, x0_cfg = R.ddim_step(noisy, e[0:1], e[1:2], ab, ab, 7.5, sds=False)
    with torch.no_grad():
        raw_cfg = R.decode(dec_sd, arch.VAE_TINY, x0_cfg)
    got = guide.preview(lat, tr.text_z, t, noise=noise.cuda(), mode='cfg')['x0']
    assert got.shape == (1, 3, res, res)
    assert float((got.cpu() - (raw_cfg / 2 + 0.5).clamp(0, 1)).abs().max()) <= 0.5 * DEC_MAX_REL * float(raw_cfg.abs().max()) + 1e-6
    assert float((x0_cfg - x0).abs().max()) > 0.1                               # (the two modes are different estimates)
    with pytest.raises(ValueError):
        guide.preview(lat, tr.text_z, t, mode='ddpm')

    losses_b += [tr.train_step(data(i % 2)) for i in range(2, 4)]
    assert tr.global_step == 4
    for (la, da), (lb, db) in zip(losses_a, losses_b):
        assert torch.equal(la, lb) and set(da) == set(db) and all(torch.equal(da[k], db[k]) for k in da)
    for n, p in model.named_parameters():
        assert torch.equal(p.detach(), params_a[n]), n
