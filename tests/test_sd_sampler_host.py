"""CPU: the host side of image sampling — the DDIM schedule (customnerf_amd.sd.sampler), the decoder's architecture table
(arch.vae_decoder_params), the seeds of the synthetic weights, and the DDIM loop of tests/vae_decoder_restatement.py on a
closed-form epsilon."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import vae_decoder_restatement as R  # noqa: E402


def test_ddim_timesteps_leading_spacing():
    from customnerf_amd.sd.sampler import ddim_timesteps
    assert ddim_timesteps(50) == list(range(981, 0, -20))
    assert ddim_timesteps(1) == [1]
    assert ddim_timesteps(500)[0] == 999 and ddim_timesteps(500)[-1] == 1
    assert ddim_timesteps(4, num_train_timesteps=10, steps_offset=0) == [6, 4, 2, 0]
    # the choice for t = T: N = 1000 with offset 1 asks for 1000 ... 1 and alphas_cumprod ends at 999 — the first timestep is CLAMPED to 999
    # (not refused), so the full-length schedule runs; everything after it is untouched
    assert ddim_timesteps(1000) == [999] + list(range(999, 0, -1))
    assert [t for t, _ in R.timesteps(50)] == ddim_timesteps(50)
    for bad in (0, 1001, -3):
        with pytest.raises(ValueError):
            ddim_timesteps(bad)


def test_ddim_schedule_previous_alpha_rule():
    from customnerf_amd.sd import arch
    from customnerf_amd.sd.sampler import ddim_schedule
    a = arch.alphas_cumprod()
    s = ddim_schedule(50, a)
    assert len(s) == 50
    assert s[0] == (981, float(a[981]), float(a[961]))
    assert s[-2] == (21, float(a[21]), float(a[1]))
    # the last step: prev = 1 - 20 < 0 -> alphas_cumprod[0], not 1 (set_alpha_to_one = False)
    assert s[-1] == (1, float(a[1]), float(a[0])) and s[-1][2] < 1.0
    # N = 1000: the clamped first step stays at alpha_bar[999]; prev comes from the unclamped t
    s = ddim_schedule(1000, a)
    assert s[0] == (999, float(a[999]), float(a[999])) and s[1] == (999, float(a[999]), float(a[998])) and s[-1] == (1, float(a[1]), float(a[0]))
    assert all(0.0 < ab <= 1.0 and 0.0 < ap <= 1.0 for _, ab, ap in s)


def _decoder_total(cfg):
    """the parameter total of AutoencoderKL's decoder half, counted from its structure (not from the table under test)"""
    conv = lambda ci, co, k: co * ci * k * k + co
    norm = lambda c: 2 * c
    resnet = lambda ci, co: norm(ci) + conv(ci, co, 3) + norm(co) + conv(co, co, 3) + (conv(ci, co, 1) if ci != co else 0)
    rev = list(reversed(cfg["block_out_channels"]))
    lc, c = cfg["latent_channels"], rev[0]
    n = conv(lc, lc, 1) + conv(lc, c, 3)
    n += 2 * resnet(c, c) + norm(c) + 4 * (c * c + c)
    prev = c
    for i, c in enumerate(rev):
        n += resnet(prev, c) + cfg["layers_per_block"] * resnet(c, c)
        if i < len(rev) - 1:
            n += conv(c, c, 3)
        prev = c
    return n + norm(c) + conv(c, cfg["in_channels"], 3)


def test_vae_decoder_params_table():
    from customnerf_amd.sd import arch
    p = arch.vae_decoder_params(arch.VAE_SD15)
    assert arch.count(p) == _decoder_total(arch.VAE_SD15) == 49_490_199
    # with the encoder half: the published size of SD-1.5's AutoencoderKL
    assert arch.count(p) + arch.count(arch.vae_encoder_params(arch.VAE_SD15)) == 83_653_863
    assert arch.count(arch.vae_decoder_params(arch.VAE_TINY)) == _decoder_total(arch.VAE_TINY)
    shapes = dict(p)
    assert len(shapes) == len(p)                                                              # no name twice
    assert shapes["post_quant_conv.weight"] == (4, 4, 1, 1) and shapes["decoder.conv_in.weight"] == (512, 4, 3, 3)
    assert shapes["decoder.conv_out.weight"] == (3, 128, 3, 3) and shapes["decoder.conv_norm_out.weight"] == (128,)
    assert shapes["decoder.mid_block.attentions.0.to_out.0.weight"] == (512, 512)
    # up blocks 512, 512, 256, 128: three resnets each, a shortcut exactly where the width changes, an upsampler on all but the last
    assert all(f"decoder.up_blocks.{i}.resnets.2.conv2.weight" in shapes for i in range(4)) and "decoder.up_blocks.0.resnets.3.conv1.weight" not in shapes
    assert shapes["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (256, 512, 1, 1)
    assert shapes["decoder.up_blocks.3.resnets.0.conv_shortcut.weight"] == (128, 256, 1, 1)
    assert [k for k in shapes if "conv_shortcut.weight" in k] == ["decoder.up_blocks.2.resnets.0.conv_shortcut.weight", "decoder.up_blocks.3.resnets.0.conv_shortcut.weight"]
    assert [f"decoder.up_blocks.{i}.upsamplers.0.conv.weight" in shapes for i in range(4)] == [True, True, True, False]
    assert not set(shapes) & set(dict(arch.vae_encoder_params(arch.VAE_SD15)))


def test_synthetic_encoder_and_unet_weights_did_not_move():
    """the decoder is seeded on its own (seed + 3): the tables and seeds of the networks that existed before give the values they gave before
    (first element and float64 sum of a few tensors, recorded on the commit before the decoder)"""
    import inspect
    from customnerf_amd.sd import arch, guidance
    enc = arch.random_state_dict(arch.vae_encoder_params(arch.VAE_TINY), 2)
    unet = arch.random_state_dict(arch.unet_params(arch.UNET_TINY), 1)
    for t, first, total in ((enc["encoder.conv_in.weight"], -0.20030228793621063, 11.481380226752663),
                            (enc["quant_conv.bias"], -0.0035192968789488077, -0.06607828289270401),
                            (unet["conv_in.weight"], -0.25426599383354187, 5.333305673196264),
                            (unet["conv_out.bias"], 0.0156619381159544, -0.015607643406838179)):
        assert float(t.flatten()[0]) == first and float(t.double().sum()) == total
    src = inspect.getsource(guidance.StableDiffusion.__init__)
    assert "arch.unet_params(self.unet_cfg), seed + 1" in src and "arch.vae_encoder_params(self.vae_cfg), seed + 2" in src and "seed + 3" in src
    dec = arch.random_state_dict(arch.vae_decoder_params(arch.VAE_TINY), 3)
    assert set(dec) == set(dict(arch.vae_decoder_params(arch.VAE_TINY))) and not set(dec) & set(enc)


@pytest.mark.parametrize("n", [5, 50])
def test_restatement_ddim_loop_recovers_x0_of_an_exact_epsilon(n):
    """with eps = (x - sqrt(ab) x0*) / sqrt(1 - ab), the noise that separates x from a fixed x0*, every step's denoised estimate is x0* and the
    loop ends close to it.  Bound: float32 round-off of (x - sb e) / sa — a few ulp of |x| / sa and of |x0*|."""
    from customnerf_amd.sd import arch
    a = arch.alphas_cumprod()
    g = torch.Generator().manual_seed(7)
    x0_star = torch.randn(2, 4, 8, 8, generator=g)
    x = torch.randn(2, 4, 8, 8, generator=g)
    seen = []

    def eps_fn(x, t):
        ab = float(a[t])
        e = (x - math.sqrt(ab) * x0_star) / math.sqrt(1 - ab)
        seen.append((t, float(x.abs().max())))
        return e, e

    out, x0s = R.ddim_loop(eps_fn, x, a, n, 7.5)
    assert len(x0s) == n and [t for t, _ in seen] == [t for t, _ in R.timesteps(n)]
    ulp = 2.0 ** -23
    for (t, xmax), x0 in zip(seen, x0s):
        bound = 16 * ulp * (xmax / math.sqrt(float(a[t])) + float(x0_star.abs().max()))
        assert float((x0 - x0_star).abs().max()) <= bound, (t, float((x0 - x0_star).abs().max()), bound)
    # after the last step x = sqrt(ab_0) x0* + sqrt(1 - ab_0) eps: within the residual noise level of x0*
    assert float((out - x0_star).abs().max()) < 0.2
