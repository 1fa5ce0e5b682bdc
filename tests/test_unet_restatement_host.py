"""CPU: what tests/test_gpu_sd_unet_stages.py rests on.

1. tests/unet_restatement.py, run in float32, is the oracle's unet_forward (1e-5 relative L2).
2. Detectability: with the fixed inputs of the GPU stage chain (UNET_TINY, loud_state_dict(seed 3), B 3, hw 16, t = 20 / 481 / 961, distinct
   x and ctx rows) every one-dimensional parameter, when dropped (bias -> 0, scale -> 1), moves the output of the block that owns it by at
   least 1.5e-2 relative L2 = 3 x the GPU tolerance of 5e-3.  A kernel that loses such a parameter is then at least d - tol >= 2 tol away from
   the float64 tap whenever its honest error is within tol.  If a seed or size change breaks this, change the inputs, not the factor.
3. Wiring faults stated as inputs of the unchanged restatement (one timestep for every row, two context rows swapped, time_emb_proj of
   neighbouring equal-width resnets swapped) move the first tap that sees them by at least the same 1.5e-2.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # sibling test modules' helpers
import unet_restatement as ur      # noqa: E402
from oracle import sd_oracle as so      # noqa: E402
from customnerf_amd.sd import arch      # noqa: E402

TOL_GPU = 5e-3
D_MIN = 3 * TOL_GPU


@pytest.fixture(scope="module")
def tiny():
    cfg = arch.UNET_TINY
    sd = ur.cast_sd(ur.loud_state_dict(arch.unet_params(cfg), 3), torch.float64)
    x, t, ctx = ur.stage_inputs(cfg, 3, 16, [20.0, 481.0, 961.0])
    with torch.no_grad():
        taps, blocks, _ = ur.chain(sd, cfg, x, t, ctx)
    return cfg, sd, (x, t, ctx), taps, blocks


@pytest.mark.parametrize("hw", [16, 24])
def test_restatement_in_float32_is_the_oracle(hw):
    cfg = arch.UNET_TINY
    sd = ur.loud_state_dict(arch.unet_params(cfg), 3)
    x, t, ctx = (v.float() for v in ur.stage_inputs(cfg, 3, hw, [20.0, 481.0, 961.0]))
    with torch.no_grad():
        ref = so.unet_forward(sd, cfg, x, t, ctx)
        taps, _, _ = ur.chain(sd, cfg, x, t, ctx)
    name, out = taps[-1]
    d = ur.rel_l2(out, ref)
    print(f"[unet restatement hw {hw}] float32 chain vs oracle: {d:.3e} relative L2")
    assert name == "out" and out.dtype == torch.float32 and d < 1e-5


def test_tap_names_follow_the_state_dict(tiny):
    cfg, sd, _, taps, _ = tiny
    names = [n for n, _ in taps]
    assert names[:3] == ["temb", "tp", "conv_in"] and names[-1] == "out" and len(set(names)) == len(names)
    for n in names[3:-1]:
        assert any(k.startswith(n) for k in sd), n
    assert [n for n in names if ".resnets." in n] == [n for n in ur.resnet_names(cfg)] and len(ur.resnet_names(cfg)) == 22
    assert sum(".attentions." in n for n in names) == 16
    assert dict(taps)["tp"].shape == (3, sum(sd[p + "time_emb_proj.bias"].numel() for p in ur.resnet_names(cfg)))


def test_every_parameter_is_audible_in_its_block(tiny):
    cfg, sd, _, taps, blocks = tiny
    with torch.no_grad():
        dist = ur.mutation_distances(sd, taps, blocks)
    n1d = sum(v.dim() == 1 for v in sd.values())
    worst = sorted(dist.items(), key=lambda kv: kv[1][1])
    for name, (tap, d) in worst[:8]:
        print(f"[unet mutation] {name} in {tap}: {d:.3e}")
    quiet = [(n, d) for n, (_, d) in dist.items() if not d >= D_MIN]
    print(f"[unet mutation] minimum distance {worst[0][1][1]:.3e} ({worst[0][0]}), {len(dist) - len(quiet)} of {n1d} one-dimensional tensors at or above {D_MIN:.1e}")
    assert n1d == len(dist) == 404
    assert not quiet, quiet


def _moved(tiny, sd=None, t=None, ctx=None):
    cfg, sd0, (x, t0, ctx0), taps, _ = tiny
    with torch.no_grad():
        mut, _, _ = ur.chain(sd if sd is not None else sd0, cfg, x, t if t is not None else t0, ctx if ctx is not None else ctx0)
    return mut


def test_row_zero_timestep_for_every_row_is_audible(tiny):
    _, _, (_, t, _), taps, _ = tiny
    mut = _moved(tiny, t=t[:1].expand(3).clone())
    name, d = ur.first_moved(taps, mut)
    print(f"[unet wiring] one timestep for all rows: {name} moves by {d:.3e}")
    assert name == "temb" and d >= D_MIN
    # and the image path hears it where the time bias first enters
    d_res = ur.rel_l2(dict(mut)["down_blocks.0.resnets.0."], dict(taps)["down_blocks.0.resnets.0."])
    print(f"[unet wiring] one timestep for all rows: down_blocks.0.resnets.0. moves by {d_res:.3e}")
    assert d_res >= D_MIN


def test_swapped_context_rows_are_audible(tiny):
    _, _, (_, _, ctx), taps, _ = tiny
    mut = _moved(tiny, ctx=ctx[[0, 2, 1]].clone())
    name, d = ur.first_moved(taps, mut)
    print(f"[unet wiring] context rows 1 and 2 swapped: {name} moves by {d:.3e}")
    assert name == "down_blocks.0.attentions.0." and d >= D_MIN


@pytest.mark.parametrize("a,b", [("down_blocks.0.resnets.0.", "down_blocks.0.resnets.1."), ("mid_block.resnets.0.", "mid_block.resnets.1."),
                                 ("down_blocks.3.resnets.0.", "down_blocks.3.resnets.1."), ("up_blocks.3.resnets.1.", "up_blocks.3.resnets.2.")])
def test_swapped_time_projections_are_audible(tiny, a, b):
    """neighbours of equal width in the stacked projection: a slice that starts one block early or late reads exactly this"""
    _, sd, _, taps, _ = tiny
    names = ur.resnet_names(tiny[0])
    assert names.index(b) == names.index(a) + 1 and sd[a + "time_emb_proj.bias"].shape == sd[b + "time_emb_proj.bias"].shape
    mut_sd = dict(sd)
    for k in ("time_emb_proj.weight", "time_emb_proj.bias"):
        mut_sd[a + k], mut_sd[b + k] = sd[b + k], sd[a + k]
    mut = _moved(tiny, sd=mut_sd)
    name, d = ur.first_moved(taps, mut)
    base, m = dict(taps), dict(mut)
    d_a, d_b = ur.rel_l2(m[a], base[a]), ur.rel_l2(m[b], base[b])
    print(f"[unet wiring] time_emb_proj of {a} and {b} swapped: {name} moves by {d:.3e}, {a} by {d_a:.3e}, {b} by {d_b:.3e}")
    assert name == "tp" and d >= D_MIN
    assert d_a >= D_MIN           # the first image tap that sees the swap
