"""CPU: the conditions under which the bound of tests/test_gpu_sd_vae_backward.py, e(got) <= 3 * e(emul) + 2**-11, keeps its power
(tests/vae_backward_testlib.py).  At the chosen inputs the rounding-faithful emulation stays close to float64 (so three times its error is
still a tight bound), it really differs from float64 (so its rounding points are applied), and an emulation that is deliberately wrong in
the way a kernel could be wrong breaks the bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the sibling testlib
import vae_backward_testlib as tl      # noqa: E402

ATTENTION_CAP = 5e-3                   # every attention tensor: six roundings deep (S, P, dP, dS and the result)
SINGLE_GEMM_CAP = 2e-3                 # a tensor one GEMM and one rounding away from its inputs


def _errors(c):
    return {name: tl.err(c.emul[name], c.ref64[name]) for name in c.emul}


@pytest.mark.parametrize("B,T,C", tl.ATTENTION_SHAPES)
def test_attention_emulation_is_close_and_mutations_break_the_bound(B, T, C):
    c = tl.attention_case(B, T, C)
    e = _errors(c)
    print(f"[attention {B}x{T}x{C}] e(emul) " + ", ".join(f"{n} {e[n]:.2e}" for n in tl.ATTENTION_TENSORS))
    for n in tl.ATTENTION_TENSORS:
        assert 0.0 < e[n] <= ATTENTION_CAP, (n, e[n])                    # > 0: the roundings are applied
    i = c.inputs
    # alpha off by 2 % in dQ only
    m = tl.attention_emul(i["q"], i["k"], i["v"], i["dO"], mutate="alpha_dq")
    e_m = tl.err(m["dQ"], c.ref64["dQ"])
    print(f"    alpha 2 % off in dQ: e {e_m:.2e} against the bound {tl.bound(e['dQ']):.2e}")
    assert e_m > tl.bound(e["dQ"])
    for n in ("O", "dK", "dV"):
        assert torch.equal(m[n], c.emul[n])
    # dS without the row centring reaches dQ and dK
    m = tl.attention_emul(i["q"], i["k"], i["v"], i["dO"], mutate="no_centring")
    for n in ("dQ", "dK"):
        e_m = tl.err(m[n], c.ref64[n])
        print(f"    dS without the centring: e({n}) {e_m:.2e} against the bound {tl.bound(e[n]):.2e}")
        assert e_m > tl.bound(e[n])


@pytest.mark.parametrize("cols,ld", tl.SOFTMAX_SHAPES)
def test_softmax_emulation_and_dispatch_table(cols, ld):
    assert ld % 8 == 0 and cols <= ld < cols + 8
    for rows in tl.SOFTMAX_ROWS:
        e = _errors(tl.softmax_case(rows, cols))
        assert 0.0 < e["P"] <= SINGLE_GEMM_CAP and 0.0 < e["dS"] <= SINGLE_GEMM_CAP, e


def test_softmax_shapes_reach_every_instantiation_with_and_without_pad():
    seen = {(tl.softmax_instantiation(ld), ld != cols) for cols, ld in tl.SOFTMAX_SHAPES}
    assert seen == {(cpl, pad) for cpl in (1, 2, 4, 8) for pad in (False, True)}
    # the dispatch rule itself, at its thresholds (so_softmax: cpl = ceil(ld / 8 / 64))
    assert [tl.softmax_instantiation(ld) for ld in (8, 512, 520, 1024, 1032, 2048, 2056, 4096)] == [1, 1, 2, 2, 4, 4, 8, 8]
    # the attention cases' own row lengths: (T, pad8(T)) -> instantiation
    assert [tl.softmax_instantiation((T + 7) // 8 * 8) for _, T, _ in tl.ATTENTION_SHAPES] == [1, 1, 2, 4, 8, 2]


@pytest.mark.parametrize("M,K,N", tl.LINEAR_SHAPES)
@pytest.mark.parametrize("residual", [False, True])
def test_linear_emulation(M, K, N, residual):
    e = _errors(tl.linear_case(M, K, N, residual))
    assert 0.0 < e["y"] <= SINGLE_GEMM_CAP and 0.0 < e["dx"] <= SINGLE_GEMM_CAP, e


def test_gemm_nt_emulation():
    e = _errors(tl.gemm_nt_case())
    assert 0.0 < e["out"] <= SINGLE_GEMM_CAP, e


@pytest.mark.parametrize("kind,B,Cin,Cout,H,W,residual", tl.CONV_CASES)
def test_conv_emulation_is_close_and_a_dropped_row_breaks_the_bound(kind, B, Cin, Cout, H, W, residual):
    c = tl.conv_case(kind, B, Cin, Cout, H, W, residual)
    e = _errors(c)
    assert 0.0 < e["y"] <= SINGLE_GEMM_CAP and 0.0 < e["dx"] <= SINGLE_GEMM_CAP, e
    if kind == "down":
        assert c.ref64["y"].shape[2:] == (H // 2, W // 2)
        assert float(c.ref64["dx"][:, :, -1, :].abs().max()) > 0 and float(c.ref64["dx"][:, :, :, -1].abs().max()) > 0     # the last row / column do receive gradient
    m = tl.conv_case(kind, B, Cin, Cout, H, W, residual, mutate="drop_last_row")
    e_m = tl.err(m.emul["dx"], c.ref64["dx"])
    print(f"[conv {kind} {B}x{Cin}x{H}x{W}] e(emul) y {e['y']:.2e} dx {e['dx']:.2e}; last input row dropped: {e_m:.2e} against {tl.bound(e['dx']):.2e}")
    assert e_m > tl.bound(e["dx"])


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 64, 128, 9, 8), (2, 256, 128, 9, 8), (2, 64, 128, 5, 7)])
@pytest.mark.parametrize("silu", [False, True])
def test_conv_groupnorm_emulation(B, Cin, Cout, H, W, silu):
    e = _errors(tl.conv_gn_case(B, Cin, Cout, H, W, silu))
    assert all(0.0 < v <= ATTENTION_CAP for v in e.values()), e          # up to four roundings deep, like the attention tensors


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 128, 128, 5, 7), (2, 128, 256, 9, 8), (2, 128, 256, 33, 31)])
def test_resnet_emulation(B, Cin, Cout, H, W):
    c = tl.resnet_case(B, Cin, Cout, H, W)
    e = _errors(c)
    print(f"[resnet {B}x{Cin}->{Cout}x{H}x{W}] e(emul) y {e['y']:.2e} dx {e['dx']:.2e}")
    assert all(0.0 < v <= ATTENTION_CAP for v in e.values()), e
    if Cin == Cout:                    # an identity skip: a gradient that leaves it out breaks the bound
        assert tl.err(c.emul["dx"] - c.inputs["dy"], c.ref64["dx"]) > tl.bound(e["dx"])
