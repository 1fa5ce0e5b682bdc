"""TEST INFRASTRUCTURE ONLY — the UNet of oracle/sd_oracle.py::unet_forward restated stage by stage (plain torch, CPU, any float dtype; the
tests run it in float64).  It is built from that module's own dtype-agnostic `resnet`, `transformer`, `_conv`, `_gn`, `_lin`; only the timestep
embedding is its own (the oracle's is pinned to float32).

`chain()` returns the ordered taps under the names UNet.forward(taps=[]) uses, and for every tap a closure f(state_dict) that recomputes just
that stage from the reference's own input to it — so the effect of one parameter is measured on the block that owns it, where it is large,
not at the end of the network, where the skip connections have drowned it (tests/test_unet_restatement_host.py).
"""
import math

import torch
import torch.nn.functional as F

from oracle import sd_oracle as so


def timestep_embedding(t, dim, dtype=torch.float64):
    """diffusers get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0) in `dtype`"""
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=dtype) / half)
    arg = t.to(dtype)[:, None] * freqs[None]
    return torch.cat([torch.cos(arg), torch.sin(arg)], dim=-1)


def cast_sd(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


class CastView:
    """read-only view of a state dict in another dtype, cast entry by entry on access (a float64 copy of the SD-1.5 weights would be 7 GB)"""

    def __init__(self, sd, dtype):
        self.sd, self.dtype = sd, dtype

    def __getitem__(self, k):
        return self.sd[k].to(self.dtype)

    def get(self, k, default=None):
        return self[k] if k in self.sd else default

    def __contains__(self, k):
        return k in self.sd


def stage_inputs(cfg, B, hw, t):
    """the inputs of the stage tests: half-rounded x [B,4,hw,hw] and ctx [B,77,D] with distinct rows from Generator(1), t as given; float64"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 4, hw, hw, generator=g).half().double()
    ctx = torch.randn(B, 77, cfg["cross_attention_dim"], generator=g).half().double()
    return x, torch.tensor(t, dtype=torch.float64), ctx


def loud_state_dict(params, seed):
    """Weights under which every one-dimensional parameter is audible in its own block: matrices as arch.random_state_dict (N(0, 1/fan_in)) and
    rounded to half (what the product stores), biases 0.5 N(0,1), every other one-dimensional tensor 1 + 0.5 N(0,1).  float32."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    sd = {}
    for name, shape in params:
        if name.endswith(".bias"):
            t = 0.5 * torch.randn(shape, generator=g)
        elif len(shape) == 1:
            t = 1.0 + 0.5 * torch.randn(shape, generator=g)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            t = (torch.randn(shape, generator=g) / math.sqrt(fan_in)).half().float()
        sd[name] = t
    return sd


def resnet_names(cfg):
    """the resnets in the order of the product's stacked time projection (UNet._resnets): down, mid, up"""
    n = len(cfg["block_out_channels"])
    L = cfg["layers_per_block"]
    return ([f"down_blocks.{i}.resnets.{j}." for i in range(n) for j in range(L)] + ["mid_block.resnets.0.", "mid_block.resnets.1."]
            + [f"up_blocks.{i}.resnets.{j}." for i in range(n) for j in range(L + 1)])


def time_projection(sd, p, temb):
    return so._lin(F.silu(temb), sd, p + "time_emb_proj")


def chain(sd, cfg, x, t, ctx):
    """x [B,4,h,w], t [B], ctx [B,77,D], all of sd's dtype -> (taps, blocks, inputs): taps = ordered [(name, tensor)], NCHW for images;
    blocks[name] = f(state_dict) -> that stage's output from the reference's input to it; inputs[name] = that input (resnets, transformers
    and convolutions: the image tensor that enters the stage, after the concat for the up path)."""
    boc, G, eps, heads = cfg["block_out_channels"], cfg["groups"], cfg["eps"], cfg["heads"]
    dtype = x.dtype
    taps, blocks, inputs = [], {}, {}

    def stage(name, f, inp=None):
        out = f(sd)
        taps.append((name, out))
        blocks[name] = f
        if inp is not None:
            inputs[name] = inp
        return out

    emb = timestep_embedding(t, boc[0], dtype)
    temb = stage("temb", lambda s: so._lin(F.silu(so._lin(emb, s, "time_embedding.linear_1")), s, "time_embedding.linear_2"))
    stage("tp", lambda s: torch.cat([time_projection(s, p, temb) for p in resnet_names(cfg)], 1))
    res = lambda p, hin: stage(p, lambda s: so.resnet(hin, temb, s, p, G, eps), hin)
    att = lambda p, hin: stage(p, lambda s: so.transformer(hin, ctx, s, p, heads, G), hin)
    h = stage("conv_in", lambda s: so._conv(x, s, "conv_in"), x)
    skips = [h]
    for i in range(len(boc)):
        for j in range(cfg["layers_per_block"]):
            h = res(f"down_blocks.{i}.resnets.{j}.", h)
            if cfg["attn_blocks"][i]:
                h = att(f"down_blocks.{i}.attentions.{j}.", h)
            skips.append(h)
        if i < len(boc) - 1:
            p = f"down_blocks.{i}.downsamplers.0.conv"
            h = stage(p + ".", lambda s, p=p, hin=h: so._conv(hin, s, p, stride=2), h)
            skips.append(h)
    h = res("mid_block.resnets.0.", h)
    h = att("mid_block.attentions.0.", h)
    h = res("mid_block.resnets.1.", h)
    attn_up = tuple(reversed(cfg["attn_blocks"]))
    for i in range(len(boc)):
        for j in range(cfg["layers_per_block"] + 1):
            h = res(f"up_blocks.{i}.resnets.{j}.", torch.cat([h, skips.pop()], dim=1))
            if attn_up[i]:
                h = att(f"up_blocks.{i}.attentions.{j}.", h)
        if i < len(boc) - 1:
            p = f"up_blocks.{i}.upsamplers.0.conv"
            h = stage(p + ".", lambda s, p=p, hin=h: so._conv(F.interpolate(hin, scale_factor=2.0, mode="nearest"), s, p), h)
    stage("out", lambda s, hin=h: so._conv(F.silu(so._gn(hin, s, "conv_norm_out", G, eps)), s, "conv_out"), h)
    return taps, blocks, inputs


def owner(name, tap_names):
    """the tap of the stage that owns state-dict entry `name`"""
    if name.startswith("time_embedding."):
        return "temb"
    if name.startswith("conv_in."):
        return "conv_in"
    if name.startswith(("conv_norm_out.", "conv_out.")):
        return "out"
    hits = [n for n in tap_names if n.endswith(".") and name.startswith(n)]
    assert len(hits) == 1, (name, hits)
    return hits[0]


def rel_l2(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


def mutation_distances(sd, taps, blocks):
    """For every one-dimensional tensor of sd: drop it (a bias becomes zero, a scale becomes one) and recompute the block that owns it from the
    reference's input -> {tensor name: (owning tap, relative L2 distance of that block's output to the unmutated one)}"""
    base = dict(taps)
    out = {}
    for name, v in sd.items():
        if v.dim() != 1:
            continue
        tap = owner(name, base.keys())
        mut = dict(sd)
        mut[name] = torch.zeros_like(v) if name.endswith(".bias") else torch.ones_like(v)
        out[name] = (tap, rel_l2(blocks[tap](mut), base[tap]))
    return out


def first_moved(taps, taps_mut):
    """(name, relative L2 distance) of the first tap that differs between two runs of the chain"""
    for (n, a), (n2, b) in zip(taps, taps_mut):
        assert n == n2
        if not torch.equal(a, b):
            return n, rel_l2(b, a)
    return None, 0.0
