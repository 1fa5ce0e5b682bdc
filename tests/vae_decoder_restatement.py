"""TEST INFRASTRUCTURE ONLY — plain-PyTorch float32 CPU restatement of the image-sampling side of the SD half: the AutoencoderKL
decoder (post_quant_conv + Decoder) and the DDIM loop (eta = 0, "leading" timesteps, steps_offset 1, set_alpha_to_one False).
Written from the public architecture with F.conv2d / F.group_norm / F.interpolate(mode='nearest') / softmax attention; it consumes
the same diffusers-named state dict as customnerf_amd.sd.vae.VAEDecoder and shares no code with the package."""
import math

import torch
import torch.nn.functional as F


def _gn(x, sd, p, G, eps):
    return F.group_norm(x, G, sd[p + ".weight"], sd[p + ".bias"], eps)


def _conv(x, sd, p, padding=1):
    return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], padding=padding)


def _resnet(x, sd, p, G, eps):
    h = _conv(F.silu(_gn(x, sd, p + "norm1", G, eps)), sd, p + "conv1")
    h = _conv(F.silu(_gn(h, sd, p + "norm2", G, eps)), sd, p + "conv2")
    if p + "conv_shortcut.weight" in sd:
        x = _conv(x, sd, p + "conv_shortcut", padding=0)
    return x + h


def decode(sd, cfg, latents):
    """latents [B, 4, h, w] (scaled) -> the decoder's raw output [B, 3, 8h, 8w] (about [-1, 1])"""
    boc, G, eps = cfg["block_out_channels"], cfg["groups"], cfg["eps"]
    z = _conv(latents / cfg["scaling_factor"], sd, "post_quant_conv", padding=0)
    h = _conv(z, sd, "decoder.conv_in")
    h = _resnet(h, sd, "decoder.mid_block.resnets.0.", G, eps)
    a = "decoder.mid_block.attentions.0."
    B, C, H, W = h.shape
    n = _gn(h, sd, a + "group_norm", G, eps).permute(0, 2, 3, 1).reshape(B, H * W, C)
    lin = lambda t, name: F.linear(t, sd[a + name + ".weight"].reshape(C, C), sd[a + name + ".bias"])
    q, k, v = lin(n, "to_q"), lin(n, "to_k"), lin(n, "to_v")
    o = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C), dim=-1) @ v
    h = h + lin(o, "to_out.0").reshape(B, H, W, C).permute(0, 3, 1, 2)
    h = _resnet(h, sd, "decoder.mid_block.resnets.1.", G, eps)
    for i in range(len(boc)):
        for j in range(cfg["layers_per_block"] + 1):
            h = _resnet(h, sd, f"decoder.up_blocks.{i}.resnets.{j}.", G, eps)
        if i < len(boc) - 1:
            h = _conv(F.interpolate(h, scale_factor=2.0, mode="nearest"), sd, f"decoder.up_blocks.{i}.upsamplers.0.conv")
    return _conv(F.silu(_gn(h, sd, "decoder.conv_norm_out", G, eps)), sd, "decoder.conv_out")


def decode_latents(sd, cfg, latents):
    """-> images [B, 3, 8h, 8w] in [0, 1]"""
    return (decode(sd, cfg, latents) / 2 + 0.5).clamp(0, 1)


def timesteps(n, T=1000, offset=1):
    """[(t, prev)]: leading spacing; prev < 0 means "before the first training step" """
    step = T // n
    return [(i * step + offset, i * step + offset - step) for i in reversed(range(n))]


def ddim_step(x, e_uncond, e_text, ab_t, ab_prev, g, sds=False):
    """-> (x_prev, x0); all arithmetic in x's dtype"""
    e = (e_text if sds else e_uncond) + g * (e_text - e_uncond)
    x0 = (x - math.sqrt(1 - ab_t) * e) / math.sqrt(ab_t)
    return math.sqrt(ab_prev) * x0 + math.sqrt(1 - ab_prev) * e, x0


def ddim_loop(eps_fn, latents, alphas, n, g):
    """eps_fn(x [B, 4, h, w], t) -> (e_uncond, e_text).  -> (latents after n steps, [x0 of every step])"""
    x, x0s = latents.clone(), []
    T = len(alphas)
    for t, prev in timesteps(n, T):
        t = min(t, T - 1)
        e_u, e_t = eps_fn(x, t)
        x, x0 = ddim_step(x, e_u, e_t, float(alphas[t]), float(alphas[max(prev, 0)]), g)
        x0s.append(x0)
    return x, x0s
