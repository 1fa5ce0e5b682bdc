"""GPU: the hand-written UNet (customnerf_amd/sd/unet.py) stage by stage against the float64 restatement tests/unet_restatement.py.

The whole-network comparison of test_gpu_sd_nets.py::test_unet_forward cannot see most one-dimensional parameters: the skip connections carry
the output, and a dropped norm bias deep in the network moves it by 2e-4 .. 3e-3, under the 5e-3 bound.  Here every tap of
UNet.forward(taps=[]) — time embedding, stacked time projection, conv_in, every resnet, transformer, down- and upsampler convolution, the
output — is compared with the float64 tap of the same name, with weights (unet_restatement.loud_state_dict) and inputs (distinct timesteps,
x rows and context rows) for which tests/test_unet_restatement_host.py shows on the CPU that every one of the 404 one-dimensional tensors,
dropped, moves its own block's output by >= 1.5e-2 = 3 x the bound used here.

Bound: 5e-3 in both metrics of test_gpu_sd_nets.rel_err (max-abs over max, relative L2), the bound the suite already uses for this network.

Measured on the MI355X, largest error over all taps per case (max-rel / L2, the tap that has it):
    stage chain tiny-16 (B 3, t 20 / 481 / 961)     1.28e-3 / 1.06e-3   up_blocks.3.attentions.0.           (out: 1.19e-3 / 0.85e-3)
    stage chain tiny-24                              1.37e-3 / 1.10e-3   down_blocks.2.attentions.1. / up_blocks.3.attentions.0.
    stage chain sd15-16 (B 2, t 20 / 961)            1.45e-3 / 1.09e-3   up_blocks.3.attentions.1. / out
    stage chain tiny-16, ops.TAIL_FUSION False       1.33e-3 / 1.07e-3   up_blocks.1.attentions.0. / up_blocks.3.attentions.0.
    temb / tp / conv_in, every case                  2.2e-4 .. 3.8e-4
    time projection slices, tiny-16 and sd15-16      1.6e-4 .. 3.2e-4 / 2.0e-4 .. 2.5e-4
    resnets on the reference's input (14 shapes)     3.2e-4 .. 6.6e-4 / 2.1e-4 .. 3.0e-4; the same bits in all six statistics combinations
    transformers on the reference's input (3 widths) 4.2e-4 .. 5.1e-4 / 3.0e-4 .. 4.6e-4; the same bits in all six, and with cached K / V
No tap came near the bound, so the chain compares every tap directly (no per-block increments), and no defect was found.
By hand, not committed: with mid_block.resnets.1.norm1.bias zeroed on the GPU side only, the final tap stays at 2.0e-3 / 1.1e-3 (the
whole-network comparison passes) while the chain fails first at mid_block.resnets.1. with 1.64e-2 / 1.65e-2.
"""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # sibling test modules' helpers
import unet_restatement as ur      # noqa: E402
from test_gpu_sd_nets import rel_err, to_nhwc8      # noqa: E402
from oracle import sd_oracle as so      # noqa: E402

TOL = 5e-3
CASES = {"tiny-16": ("tiny", 3, 16, (20.0, 481.0, 961.0)), "tiny-24": ("tiny", 3, 24, (20.0, 481.0, 961.0)), "sd15-16": ("sd15", 2, 16, (20.0, 961.0))}


class Case:
    """weights, inputs and the float64 chain of one case; computed once and never modified"""

    def __init__(self, key):
        from customnerf_amd.sd import arch
        cfg_name, B, hw, t = CASES[key]
        self.key, self.cfg = key, arch.UNET_TINY if cfg_name == "tiny" else arch.UNET_SD15
        self.sd = ur.loud_state_dict(arch.unet_params(self.cfg), 3)                    # float32, matrices on the half grid: what the product is given
        self.sd64 = ur.CastView(self.sd, torch.float64)
        self.x, self.t, self.ctx = ur.stage_inputs(self.cfg, B, hw, list(t))
        with torch.no_grad():
            self.taps, self.blocks, self.inputs = ur.chain(self.sd64, self.cfg, self.x, self.t, self.ctx)
        self.ref = dict(self.taps)

    def gpu_inputs(self):
        return to_nhwc8(self.x), self.t.float().cuda(), self.ctx.half().cuda()


@functools.lru_cache(maxsize=None)
def case(key):
    return Case(key)


@functools.lru_cache(maxsize=None)
def network(key):
    from customnerf_amd.sd.unet import UNet
    c = case(key)
    return UNet(c.cfg, c.sd, "cuda")


def nchw(v):
    return v.permute(0, 3, 1, 2) if v.dim() == 4 else v


def compare_taps(tag, got, c):
    """print both errors of every tap, then assert the bound for all of them"""
    assert [n for n, _ in got] == [n for n, _ in c.taps]
    bad, worst = [], (0.0, 0.0, None, None)
    for (name, g), (_, r) in zip(got, c.taps):
        assert nchw(g).shape == r.shape, (name, g.shape, r.shape)
        emax, el2 = rel_err(nchw(g).double(), r)
        print(f"[unet stages {tag}] {name:<40} max rel {emax:.3e}  L2 rel {el2:.3e}  (max |ref| {float(r.abs().max()):.1f})")
        worst = (max(worst[0], emax), max(worst[1], el2), name if emax > worst[0] else worst[2], name if el2 > worst[1] else worst[3])
        if not (emax < TOL and el2 < TOL):
            bad.append((name, emax, el2))
    print(f"[unet stages {tag}] largest: max rel {worst[0]:.3e} at {worst[2]}, L2 rel {worst[1]:.3e} at {worst[3]}")
    assert not bad, f"[{tag}] first tap out of bound: {bad[0]}; all: {bad}"


def run_chain(key):
    c, net = case(key), network(key)
    taps = []
    with torch.no_grad():
        out = net(*c.gpu_inputs(), taps=taps)
    assert taps[-1][1] is out and taps[1][0] == "tp" and taps[1][1].dtype == torch.float32
    return taps, out


# ------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("key", ["tiny-16", "tiny-24", "sd15-16"])
def test_stage_chain(key):
    """tiny-16: 256 / 64 / 16 / 4 rows per image, so both the admissible (>= 64 rows) and the refused GroupNorm-epilogue routes of ops._attach_gn
    and the concat-statistics route run; tiny-24: 576 / 144 / 36 / 9 rows; sd15-16: the GEMM plans, split-K and LayerNorm-tail routes that
    320 .. 1280 channels select and 128 .. 384 do not."""
    taps, _ = run_chain(key)
    compare_taps(key, taps, case(key))


def test_stage_chain_without_tail_fusion(monkeypatch):
    """the stand-alone statistics / LayerNorm launches (ops.TAIL_FUSION False) compute the same network"""
    from customnerf_amd.sd import ops
    monkeypatch.setattr(ops, "TAIL_FUSION", False)
    taps, _ = run_chain("tiny-16")
    compare_taps("tiny-16 no tail fusion", taps, case("tiny-16"))


def resnets_by_name(net):
    out = {}
    for i, (res, _, _) in enumerate(net.down):
        out.update({f"down_blocks.{i}.resnets.{j}.": r for j, r in enumerate(res)})
    out.update({"mid_block.resnets.0.": net.mid[0], "mid_block.resnets.1.": net.mid[2]})
    for i, (res, _, _) in enumerate(net.up):
        out.update({f"up_blocks.{i}.resnets.{j}.": r for j, r in enumerate(res)})
    return out


@pytest.mark.parametrize("key", ["tiny-16", "sd15-16"])
def test_time_projection_slices(key):
    """every resnet's [t_off, t_off + t_n) slice of the stacked projection is time_emb_proj(silu(temb)) of the resnet of that name, and the
    slices tile the projection without gap or overlap"""
    c, net = case(key), network(key)
    taps, _ = run_chain(key)
    tp = dict(taps)["tp"]
    named = resnets_by_name(net)
    assert set(named) == set(ur.resnet_names(c.cfg)) and {id(r) for r in named.values()} == {id(r) for r in net._resnets}
    bad = []
    for name, r in named.items():
        ref = ur.time_projection(c.sd64, name, c.ref["temb"])
        assert r.t_n == ref.shape[1], name
        emax, el2 = rel_err(tp[:, r.t_off:r.t_off + r.t_n].double(), ref)
        print(f"[unet tp {key}] {name:<28} columns {r.t_off:>5} .. {r.t_off + r.t_n:>5}  max rel {emax:.3e}  L2 rel {el2:.3e}")
        if not (emax < TOL and el2 < TOL):
            bad.append((name, emax, el2))
    assert not bad, bad
    end = 0
    for r in sorted(named.values(), key=lambda r: r.t_off):
        assert r.t_off == end, "gap or overlap in the stacked time projection"
        end += r.t_n
    assert end == tp.shape[1]


# ------------------------------------------------------------------------------------------------ blocks on the reference's input
def _tiny_block_shapes():
    """one resnet per distinct (input width, output width, rows) of UNET_TINY at hw 16 — with and without conv_shortcut, concat widths — and one
    transformer per width"""
    from customnerf_amd.sd import arch
    cfg = arch.UNET_TINY
    boc, L = cfg["block_out_channels"], cfg["layers_per_block"]
    res, att, cin, hw = {}, {}, boc[0], 16
    for i, c in enumerate(boc):
        for j in range(L):
            res.setdefault((cin, c, hw), f"down_blocks.{i}.resnets.{j}.")
            if cfg["attn_blocks"][i]:
                att.setdefault((c, hw), f"down_blocks.{i}.attentions.{j}.")
            cin = c
        if i < len(boc) - 1:
            hw //= 2
    res.setdefault((boc[-1], boc[-1], hw), "mid_block.resnets.0.")
    for i, blk in enumerate(arch.unet_up_channels(cfg)):
        for j, (rin, skip, oc) in enumerate(blk):
            res.setdefault((rin + skip, oc, hw), f"up_blocks.{i}.resnets.{j}.")
        if i < len(boc) - 1:
            hw *= 2
    return sorted(res.values()), sorted(att.values())


RESNETS, TRANSFORMERS = _tiny_block_shapes()
COMBOS = [(xs, og) for xs in ("absent", "given", "unfilled") for og in (False, True)]


def nhwc_half(x):
    return x.permute(0, 2, 3, 1).contiguous().half().cuda()


def check_block(tag, groups, run, ref, norm_w, norm_b, eps, silu):
    """run(x_sums, out_gn) -> (y, y_sums | None) for every way the block can be handed / asked for GroupNorm statistics: the outputs are the same
    bits (the statistics of x are the norm kernel's own in every case, and a statistics request does not change what a GEMM writes), within
    TOL of the float64 block, and returned statistics are those of the returned tensor."""
    from customnerf_amd.sd import ops
    x = run.x
    first = None
    for xs, og in COMBOS:
        if xs == "absent":
            x_sums = None
        elif xs == "given":                                      # the statistics of x, ready (as a producing GEMM would leave them)
            x_sums = (ops.groupnorm(x, norm_w, norm_b, groups, eps, silu)[1], True)
        else:                                                    # a pre-zeroed buffer the producer did not fill
            x_sums = (torch.zeros(x.shape[0], groups, 2, dtype=torch.int64, device="cuda"), False)
        y, ys = run(x_sums, og)
        emax, el2 = rel_err(nchw(y).double(), ref)
        print(f"[unet block {tag}] x_sums {xs:<8} out_gn {og!s:<5} max rel {emax:.3e}  L2 rel {el2:.3e}" + (f"  statistics returned ready: {ys[1]}" if og else ""))
        assert emax < TOL and el2 < TOL, (tag, xs, og, emax, el2)
        if first is None:
            first = y.clone()
        assert torch.equal(y, first), (tag, xs, og)
        assert (ys is not None) == og
        if og:
            sums, ok = ys
            B, H, W, C = y.shape
            assert ok == (H * W >= 64), "the GroupNorm-epilogue request is admissible from 64 rows per image (ops._attach_gn)"
            if ok:
                yg = y.double().view(B, H * W, groups, C // groups)
                want = torch.stack([yg.sum((1, 3)), (yg * yg).sum((1, 3))], -1)
                # the tolerance of test_gpu_sd_ops.py::test_gemm_fused_groupnorm_statistics
                torch.testing.assert_close(ops.gn_sums_to_float(sums).float().cpu(), want.float().cpu(), rtol=2e-4, atol=1e-2)
            else:
                assert not bool(sums.any()), "a refused request leaves the pre-zeroed buffer for the consuming norm to fill"


@pytest.mark.parametrize("name", RESNETS)
def test_resnet_on_reference_input(name):
    from customnerf_amd.sd import ops
    from customnerf_amd.sd.unet import _Resnet
    c = case("tiny-16")
    G, eps = c.cfg["groups"], c.cfg["eps"]
    xin = c.inputs[name].half()                                   # the float64 tap that precedes the block, rounded to half
    tb64 = ur.time_projection(c.sd64, name, c.ref["temb"])
    with torch.no_grad():
        ref = so.resnet(xin.double(), c.ref["temb"], c.sd64, name, G, eps)
    r = _Resnet(c.sd, name, torch.device("cuda"))
    assert r.has_sc == (xin.shape[1] != ref.shape[1])
    # the reference projection as forward() hands it over: a strided view into a wider float32 matrix, at a non-zero column offset
    off = 24
    wide = torch.full((xin.shape[0], off + tb64.shape[1] + 40), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, off:off + tb64.shape[1]] = tb64.float().cuda()
    tb = wide[:, off:off + tb64.shape[1]]
    assert tb.stride(0) != tb.shape[1] and tb.storage_offset() == off

    def run(x_sums, out_gn):
        return r(run.x, tb, G, eps, ops.SumsPool(8, xin.shape[0], G, "cuda"), x_sums=x_sums, out_gn=out_gn)
    run.x = nhwc_half(xin)
    check_block(f"{name} {xin.shape[1]} -> {ref.shape[1]} at {xin.shape[2]}^2", G, run, ref, r.n1w, r.n1b, eps, True)


@pytest.mark.parametrize("name", TRANSFORMERS)
def test_transformer_on_reference_input(name):
    from customnerf_amd.sd import ops
    from customnerf_amd.sd.unet import _Transformer
    c = case("tiny-16")
    G = c.cfg["groups"]
    xin = c.inputs[name].half()
    with torch.no_grad():
        ref = so.transformer(xin.double(), c.ctx, c.sd64, name, c.cfg["heads"], G)
    a = _Transformer(c.sd, name, torch.device("cuda"), c.cfg["heads"])
    ctx = c.ctx.half().cuda()

    def run(x_sums, out_gn):
        return a(run.x, ctx, G, ops.SumsPool(8, xin.shape[0], G, "cuda"), x_sums=x_sums, out_gn=out_gn)
    run.x = nhwc_half(xin)
    check_block(f"{name} {xin.shape[1]} at {xin.shape[2]}^2", G, run, ref, a.nw, a.nb, 1e-6, False)
    y, _ = run(None, False)
    y_kv, _ = a(run.x, None, G, ops.SumsPool(8, xin.shape[0], G, "cuda"), kv=a.context_kv(ctx))
    assert torch.equal(y_kv, y)


# ------------------------------------------------------------------------------------------------ context cache and graphs
def test_context_cache_and_graphs():
    """cached cross-attention K / V, the per-context graphs and their 4-entry LRU give the eager forward's bits for the context they are asked
    for; recording taps does not change the output"""
    c, net = case("tiny-16"), network("tiny-16")
    x, t, ctx = c.gpu_inputs()
    g = torch.Generator().manual_seed(7)
    others = [torch.randn(ctx.shape, generator=g).half().cuda() for _ in range(5)]
    with torch.no_grad():
        out = net(x, t, ctx).clone()
        assert torch.equal(run_chain("tiny-16")[1], out)
        assert torch.equal(net(x, t, None, ctx_kv=net.context_kv(ctx)), out)
        eager = [net(x, t, o).clone() for o in others]
        assert not torch.equal(eager[0], out) and not torch.equal(eager[0], eager[1])
        for _ in range(2):                                        # two contexts in turn: the second round replays
            assert torch.equal(net.graphed(x, t, ctx), out)
            assert torch.equal(net.graphed(x, t, others[0]), eager[0])
        assert len(net._graph) == 2
        ctx2 = ctx.clone()
        assert torch.equal(net.graphed(x, t, ctx2), out)
        ctx2.mul_(0.5)                                            # same storage, new version: the cached K / V and graph are stale
        assert torch.equal(net.graphed(x, t, ctx2), net(x, t, ctx2))
        for o, e in zip(others, eager):                           # five contexts through four slots
            assert torch.equal(net.graphed(x, t, o), e)
        assert len(net._graph) == 4
        assert torch.equal(net.graphed(x, t, others[0]), eager[0])            # evicted above, captured again
        assert torch.equal(net.graphed(x, t, ctx), out)
        assert torch.equal(net.graphed(x * 0.5, t.flip(0), others[4]), net(x * 0.5, t.flip(0), others[4]))      # a replay with new x and t
    net._graph = None
