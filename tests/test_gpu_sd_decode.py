"""GPU: latents -> image.  customnerf_amd.sd.vae.VAEDecoder (float16 activations on the HIP primitives) against the float32 CPU
restatement tests/vae_decoder_restatement.py on the same half-rounded weights, the two glue kernels at its ends
(cnerf_sd_decoder_input / cnerf_sd_decoder_output) against their formulas, and StableDiffusion.decode_latents."""
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

# float16 activations through the decoder's ~45 layers against the float32 restatement, relative to the output's own scale.
# Measured on MI355X (max rel / L2 rel): tiny 8x8 1.10e-3 / 0.98e-3, tiny 2x8x12 1.27e-3 / 1.01e-3, SD-1.5 shapes 16x16 1.02e-3 / 1.07e-3;
# bounds = 3 x the largest
DEC_MAX_REL, DEC_L2_REL = 3.8e-3, 3.2e-3


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12)), float((a - b).norm() / (b.norm() + 1e-12))


def half_sd(sd):
    """the product stores weights as float16: give the restatement the same (rounded) values"""
    return {k: (v.half().float() if v.dim() > 1 else v) for k, v in sd.items()}


@pytest.mark.parametrize("cfg_name,shape", [("tiny", (1, 4, 8, 8)), ("tiny", (2, 4, 8, 12)), ("sd15", (1, 4, 16, 16))])
def test_vae_decoder_matches_restatement(cfg_name, shape):
    from customnerf_amd.sd import arch
    from customnerf_amd.sd.vae import VAEDecoder
    cfg = arch.VAE_TINY if cfg_name == "tiny" else arch.VAE_SD15
    sd = half_sd(arch.random_state_dict(arch.vae_decoder_params(cfg), seed=7))
    g = torch.Generator().manual_seed(shape[2] * 100 + shape[3])
    lat = torch.randn(shape, generator=g)                                       # unit-variance latents, as encode_imgs scales them
    with torch.no_grad():
        ref = R.decode(sd, cfg, lat)
    dec = VAEDecoder(cfg, sd, "cuda")
    raw = dec(lat.cuda())
    B, _, h, w = shape
    assert raw.shape == (B, 8 * h, 8 * w, 8) and raw.dtype == torch.float16
    assert not raw[..., 3:].any()                                               # conv_out's padding filters
    emax, el2 = rel_err(raw[..., :3].permute(0, 3, 1, 2), ref)
    print(f"[vae decoder {cfg_name}-{tuple(shape)}] max rel {emax:.3e}, L2 rel {el2:.3e}; |ref| max {float(ref.abs().max()):.3f}")
    assert emax < DEC_MAX_REL and el2 < DEC_L2_REL, (emax, el2)
    img, u8 = dec.decode(lat.cuda(), image=True, image_u8=True)
    assert img.shape == (B, 3, 8 * h, 8 * w) and img.dtype == torch.float32 and u8.shape == (B, 8 * h, 8 * w, 3) and u8.dtype == torch.uint8
    ref_img = (ref / 2 + 0.5).clamp(0, 1)
    assert float((img.cpu() - ref_img).abs().max()) <= 0.5 * DEC_MAX_REL * float(ref.abs().max()) + 1e-6
    assert 0.0 <= float(img.min()) and float(img.max()) <= 1.0
    assert torch.equal(u8, (255.0 * img).round().to(torch.uint8).permute(0, 2, 3, 1))


def test_vae_decoder_accepts_old_attention_names():
    from customnerf_amd.sd import arch
    from customnerf_amd.sd.vae import VAEDecoder
    cfg = arch.VAE_TINY
    sd = arch.random_state_dict(arch.vae_decoder_params(cfg), seed=7)
    old = {}
    for k, v in sd.items():
        for o, n in arch.VAE_ATTN_ALIASES.items():
            if k.startswith("decoder.mid_block.attentions.0." + n + "."):
                k = k.replace("attentions.0." + n + ".", "attentions.0." + o + ".")
                v = v[:, :, None, None] if v.dim() == 2 else v                  # the old checkpoints hold them as 1x1 convolutions
        old[k] = v
    assert "decoder.mid_block.attentions.0.proj_attn.weight" in old and "decoder.mid_block.attentions.0.to_q.weight" not in old
    lat = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(1)).cuda()
    assert torch.equal(VAEDecoder(cfg, old, "cuda")(lat), VAEDecoder(cfg, sd, "cuda")(lat))


def test_decoder_input_kernel():
    """cnerf_sd_decoder_input against (lat / s) @ W^T + b in float64: equal after rounding to half up to one half-ulp; padding exactly zero"""
    from customnerf_amd.sd import ops
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(3, 4, 5, 7, generator=g)                                  # odd sizes, more than one image, not a multiple of the wave
    W, b = torch.randn(4, 4, generator=g), torch.randn(4, generator=g)
    s = 0.18215
    out = ops.decoder_input(lat.cuda(), torch.cat([W.flatten(), b]).cuda(), s).cpu()
    assert out.shape == (3, 5, 7, 8) and out.dtype == torch.float16
    assert not out[..., 4:].any()
    s32 = float(torch.tensor(s, dtype=torch.float32))                           # the scale as the kernel receives it
    ref = torch.einsum("bihw,oi->bhwo", lat.double() / s32, W.double()) + b.double()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14))) - 10)
    assert bool(((out[..., :4].double() - ref).abs() <= ulp).all())
    # a 128 x 128 latent: more than one block per image
    big = torch.randn(1, 4, 128, 128, generator=g)
    out = ops.decoder_input(big.cuda(), torch.cat([W.flatten(), b]).cuda(), s).cpu()
    ref = torch.einsum("bihw,oi->bhwo", big.double() / s32, W.double()) + b.double()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14))) - 10)
    assert bool(((out[..., :4].double() - ref).abs() <= ulp).all()) and not out[..., 4:].any()


@pytest.mark.parametrize("ld", [3, 4, 8])
def test_decoder_output_kernel(ld):
    """float image within 1e-6 of clamp(x / 2 + 0.5, 0, 1) on the half input, uint8 image exactly round(255 x that), values outside [-1, 1] clamp"""
    from customnerf_amd.sd import ops
    g = torch.Generator().manual_seed(ld)
    x = (torch.randn(2, 5, 7, ld, generator=g) * 0.8).half()
    x[0, 0, 0, :3] = torch.tensor([-1.0, 1.0, 0.0]).half()
    x[0, 0, 1, :3] = torch.tensor([-3.5, 2.25, 65504.0]).half()
    x[1, 4, 6, :3] = torch.tensor([-65504.0, 1.0009765625, -1.0009765625]).half()
    assert int((x[..., :3].float().abs() > 1).sum()) > 10                     # both clamps are exercised well beyond the hand-set pixels
    img, u8 = ops.decoder_output(x.cuda(), image=True, image_u8=True)
    ref = (x[..., :3].float() / 2 + 0.5).clamp(0, 1).permute(0, 3, 1, 2)
    assert img.shape == (2, 3, 5, 7) and float((img.cpu() - ref).abs().max()) <= 1e-6
    assert img[0, :, 0, 0].tolist() == [0.0, 1.0, 0.5] and img[0, :, 0, 1].tolist() == [0.0, 1.0, 1.0] and img[1, :, 4, 6].tolist() == [0.0, 1.0, 0.0]
    assert u8.shape == (2, 5, 7, 3) and torch.equal(u8, (255.0 * img).round().to(torch.uint8).permute(0, 2, 3, 1))
    # each output on its own
    only_img, none = ops.decoder_output(x.cuda(), image=True, image_u8=False)
    none2, only_u8 = ops.decoder_output(x.cuda(), image=False, image_u8=True)
    assert none is None and none2 is None and torch.equal(only_img, img) and torch.equal(only_u8, u8)


def test_decode_latents_is_lazy_reproducible_and_needs_decoder_weights():
    from customnerf_amd.sd import arch
    from customnerf_amd.sd.guidance import StableDiffusion
    opt = types.SimpleNamespace(cfg=7.5, lambda_sd=0.01, max_ratio=0.98, stage_time=False, iters=10, log_loss_item=False)
    guide = StableDiffusion("cuda", "1.5", opt, unet_cfg=arch.UNET_TINY, vae_cfg=arch.VAE_TINY, seed=4)
    assert guide._vae_dec is None                                               # built on first use
    lat = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(0)).cuda()
    a = guide.decode_latents(lat)
    assert guide._vae_dec is not None
    b = guide.decode_latents(lat)
    assert a.shape == (2, 3, 64, 64) and a.dtype == torch.float32 and torch.equal(a, b)
    # synthetic mode: the decoder's own seed (seed + 3)
    sd = half_sd(arch.random_state_dict(arch.vae_decoder_params(arch.VAE_TINY), 4 + 3))
    with torch.no_grad():
        ref = R.decode(sd, arch.VAE_TINY, lat.cpu())
    assert float((a.cpu() - (ref / 2 + 0.5).clamp(0, 1)).abs().max()) <= 0.5 * DEC_MAX_REL * float(ref.abs().max()) + 1e-6
    # an encoder-only state dict: constructing works as before, the first decode says what is missing
    enc_only = arch.random_state_dict(arch.vae_encoder_params(arch.VAE_TINY), 2)
    guide2 = StableDiffusion("cuda", "1.5", opt, unet_state=arch.random_state_dict(arch.unet_params(arch.UNET_TINY), 1), vae_state=enc_only,
                             unet_cfg=arch.UNET_TINY, vae_cfg=arch.VAE_TINY)
    with pytest.raises(ValueError, match="decoder"):
        guide2.decode_latents(lat)
