"""CPU: the probes of tests/test_gpu_sd_gemm.py are sound and have teeth (tests/gemm_restatement.py).

  * `reference`, the int64 / float64 restatement of the cnerf_sd_gemm contract, agrees exactly with torch's float64 conv2d (forward cells),
    interpolate(nearest) + conv2d (ups cells), autograd's input gradient (dgrad cells) and A @ B.T (dense cells), epilogue included;
  * every builder meets its exactness conditions on every cell, in both layouts (the builders assert them; here also the layout itself:
    NaN everywhere outside the problem, the ragged edges non-zero), and the float32 identities the GEGLU pairing probe rests on hold;
  * `model`, a kernel of csrc/sd_gemm.hip's structure in numpy (tiles, 8-column chunks, 64-wide K steps, kps splits, the uniform tap state
    initialised at a split's first K step, bucketed statistics), passes every check on every cell;
  * each of thirteen seeded defects of `model` fails at least one probe.  test_each_seeded_defect_is_caught prints the table:

        drop_last_ragged_k_chunk            field     dense-130x72x40, dense-130x72x200, split-77x328x1160
        split_tap_state_channel_0           field     conv-split-c128-8x8
        kh_kw_swapped                       field     conv-c8-9x7, conv-c64-9x7
        pad_l_for_pad_t                     field     conv-c16-pad-2-1-9x7, conv-c64-pad-2-1-9x7
        odd_tstride_taps_kept               field     conv-c136 / c48 / c128 / c64 dgrad cells (both loaders)
        ups_floor_before_sign_test          field     conv-c72-ups-5x3, conv-c64-ups-5x3
        image_bias_row_of_tile_start        field     conv-c64-b3-5x4-image-bias
        residual_pitch_ldc                  poison    dense-130x72x200, dense-257x136x320 (NaN from the pad of ldr)
        geglu_pair_shifted                  pairing   geglu-77x128x16
        full_store_on_ragged_chunk          sentinel  heads-d24, dense-33x75x72
        third_group_folded_into_second      stats     gn-cg5, gn-g6-cg5, gn-rows100-cg5, gn-conv-c64-b3-8x8-cg5
        stats_second_image_to_first         stats     gn-cg4, gn-rows100-cg5
        split_partial_left_out              field     split-128x64x1024, split-64x64x1216
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the sibling library
import gemm_restatement as gr      # noqa: E402

IDS = [c.name for c in gr.ALL_CELLS]
_PROBES = {}


def probe(cell, padded):
    """built once per session and shared, never modified"""
    key = (cell.name, padded)
    if key not in _PROBES:
        _PROBES[key] = gr.build(cell, padded)
    return _PROBES[key]


def _epilogue64(p, v):
    """the epilogue in torch float64 on v [M, N], from the probe's LOGICAL values (a second route to them than reference()'s buffer reads)"""
    c = p.cell
    M, N = p.M, p.N
    v = c.alpha * v
    if p.bias is not None:
        v = v + torch.from_numpy(p.bias).double()[None]
    if p.br_buf is not None:
        br = torch.from_numpy(p.br_buf).double().view(-1, p.ld_bias_rows)[:, :N]
        v = v + br[torch.arange(M) // c.bias_rows]
    if c.act == gr.ACT_GEGLU:
        v = v[:, 0::2] * torch.nn.functional.gelu(v[:, 1::2])
    if p.r_buf is not None:
        v = v + torch.from_numpy(p.r_buf[p.r_off:p.r_off + M * p.ldr].astype(np.float64)).view(M, p.ldr)[:, :N]
    return v


@pytest.mark.parametrize("cell", gr.ALL_CELLS, ids=IDS)
def test_restatement_is_torch_float64(cell):
    p = probe(cell, True)
    c = cell.conv
    if cell.heads is not None:
        Bt, heads, d, Tq, Tk = cell.heads
        q = torch.from_numpy(p.logical["q"]).double().view(Bt, Tq, heads, d).transpose(1, 2)
        k = torch.from_numpy(p.logical["k"]).double().view(Bt, Tk, heads, d).transpose(1, 2)
        want = cell.alpha * (q @ k.transpose(2, 3)).reshape(Bt * heads, Tq, Tk)
    elif c is None:
        want = _epilogue64(p, torch.from_numpy(p.logical["A"]).double() @ torch.from_numpy(p.logical["B"]).double().T)[None]
    else:
        x = torch.from_numpy(p.logical["x"]).double().permute(0, 3, 1, 2)                  # NCHW
        w = torch.from_numpy(p.logical["B"]).double().view(c.Cout, c.KH, c.KW, c.Cin)      # packed (kh, kw, ci)
        Ho, Wo = c.hw_out()
        if c.tstride == 2:
            # the input gradient of conv2d(F.pad(u, (0, e, 0, e)), W, stride s, padding q) at dy = x.  B = W flipped and transposed:
            # B[ci][kh][kw][co] = W[co][ci][KH - 1 - kh][KW - 1 - kw], pad = KH - 1 - q, tstride = s
            s, q_, e = c.fwd
            assert (c.stride, c.pad_t, c.pad_l, c.tstride) == (1, c.KH - 1 - q_, c.KW - 1 - q_, s)
            W = w.flip(1, 2).permute(3, 0, 1, 2).contiguous()                              # [co_f = Cin, ci_f = Cout, KH, KW]
            u = torch.zeros(c.B, c.Cout, Ho, Wo, dtype=torch.float64, requires_grad=True)
            yf = torch.nn.functional.conv2d(torch.nn.functional.pad(u, (0, e, 0, e)), W, stride=s, padding=q_)
            assert yf.shape == x.shape, "the dgrad cell's input is the forward conv's output"
            yf.backward(x)
            y = u.grad
        else:
            if c.ups == 2:
                x = torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")
            Hn, Wn = (Ho - 1) * c.stride + c.KH, (Wo - 1) * c.stride + c.KW                # the window the outputs cover: zero beyond the input
            x = torch.nn.functional.pad(x, (c.pad_l, max(Wn - x.shape[3] - c.pad_l, 0), c.pad_t, max(Hn - x.shape[2] - c.pad_t, 0)))
            y = torch.nn.functional.conv2d(x, w.permute(0, 3, 1, 2), stride=c.stride)[:, :, :Ho, :Wo]
            assert y.shape[2:] == (Ho, Wo)
        want = _epilogue64(p, y.permute(0, 2, 3, 1).reshape(p.M, p.N))[None]
    assert np.array_equal(p.expect, want.numpy()), f"{cell.name}: the restatement differs from torch float64"
    if cell.gn:
        groups, rows = cell.gn
        h = want[0].view(p.M // rows, rows, groups, p.N // groups)
        assert np.array_equal(p.expect_sums[..., 0], (h.sum((1, 3)) * 2 ** gr.FRAC_BITS).long().numpy())
        assert np.array_equal(p.expect_sums[..., 1], ((h * h).sum((1, 3)) * 2 ** gr.FRAC_BITS).long().numpy())


@pytest.mark.parametrize("cell", gr.ALL_CELLS, ids=IDS)
def test_builders_meet_their_conditions(cell):
    """build() runs _assert_exact; here the layout: same values in both forms, NaN everywhere a correct kernel never reads, ragged edges alive"""
    t, p = probe(cell, False), probe(cell, True)
    assert np.array_equal(t.expect, p.expect) and (cell.gn is None or np.array_equal(t.expect_sums, p.expect_sums))
    assert p.a_buf.dtype == p.b_buf.dtype == np.float16
    assert not np.isnan(t.a_buf).any() and not np.isnan(t.b_buf).any()
    if cell.heads is None:
        b = p.b_buf.reshape(-1, p.ldb)
        assert p.ldb > p.K and np.isnan(b[:, p.K:]).all() and np.isnan(b[p.N:]).all() and b.shape[0] > p.N
        assert (b[p.N - 1, :p.K] != 0).any() and (b[:p.N, p.K - 8:p.K] != 0).any()
        if cell.conv is None:
            a = p.a_buf.reshape(-1, p.lda)
            assert p.lda > p.K and np.isnan(a[:, p.K:]).all() and np.isnan(a[p.M:]).all() and a.shape[0] > p.M
            assert (a[p.M - 1, :p.K] != 0).all() and (a[:p.M, p.K - 8:p.K] != 0).any(1).all()
        else:
            c = cell.conv
            n = c.B * c.H * c.W * c.Cin
            x = p.a_buf[:n].reshape(c.B, c.H, c.W, c.Cin)
            assert p.a_buf.size >= n + 2 * c.W * c.Cin and np.isnan(p.a_buf[n:]).all()
            assert (x[:, [0, -1]] != 0).all() and (x[:, :, [0, -1]] != 0).all(), "border pixels carry non-zero operands"
            assert c.H != c.W or cell not in gr.CONV_CHUNK + gr.CONV_UNIFORM, "non-square images"
        if cell.residual:
            r = p.r_buf[p.r_off:].reshape(-1, p.ldr)
            assert p.ldr > p.N and p.ldr != p.ldc and np.isnan(r[:, p.N:]).all() and np.isnan(r[p.M:]).all()
        if cell.bias_rows:
            br = p.br_buf.reshape(-1, p.ld_bias_rows)
            n_img = -(-p.M // cell.bias_rows)
            assert p.ld_bias_rows > p.N and np.isnan(br[:, p.N:]).all() and np.isnan(br[n_img:]).all()
            assert all(not np.array_equal(br[i, :p.N], br[j, :p.N]) for i in range(n_img) for j in range(i))
        assert cell.plain_ldc or p.ldc > p.width
        assert p.c_elems > p.M * p.ldc
    else:
        assert p.ldc == gr.pad8(cell.heads[4]) > p.N
    C, C32, gn = p.outputs()
    assert (C.view(np.uint16) == gr.SENT16).all() and (C32.view(np.uint32) == gr.SENT32).all() and C.size == p.c_elems
    assert float(C[0]) != round(float(C[0])), "the sentinel is no value an integer probe can produce"


def test_geglu_identities_in_float32():
    """what the pairing probe rests on: with the kernel's float32 formula gelu(16) == 16 and gelu(0) == 0 exactly, gelu of a small non-zero
    integer is no integer"""
    f = np.float32

    def gelu32(g):
        return f(f(f(0.5) * f(g)) * f(f(1.0) + f(math.erf(float(f(f(g) * f(0.70710678118654752)))))))
    assert gelu32(16.0) == f(16.0) and gelu32(0.0) == f(0.0)
    for v in (-3, -2, -1, 1, 2, 3):
        assert gelu32(float(v)) != np.rint(gelu32(float(v)))
    for cell in gr.GEGLU:
        p = probe(cell, True)
        A, B = p.logical["A"], p.logical["B"]
        pre = A @ B.T + p.bias.astype(np.int64)[None]
        if cell.bias_rows:
            pre = pre + p.br_buf.reshape(-1, p.ld_bias_rows)[np.arange(p.M) // cell.bias_rows, :p.N].astype(np.int64)
        gate, val = pre[:, 1::2], pre[:, 0::2]
        assert set(np.unique(gate)) == {0, 16}, "the gate pre-activation is 0 or 16"
        assert np.array_equal(p.expect[0], (val * gate).astype(np.float64)) and np.abs(val).max() <= 128
        assert (val != 0).mean() > 0.5 and (np.abs(val) <= 3).any()


def _splits(cell):
    return 2 if cell.split else 1


@pytest.mark.parametrize("cell", gr.ALL_CELLS, ids=IDS)
def test_model_passes_every_check(cell):
    for padded in (False, True):
        p = probe(cell, padded)
        for bn in (64, 128):
            assert gr.check(p, *gr.model(p, _splits(cell), bn)) is None
    if cell.split:
        p = probe(cell, True)
        assert gr.check(p, *gr.model(p, 3, 64)) is None


CANDIDATES = {
    "drop_last_ragged_k_chunk": ["dense-130x72x40", "dense-130x72x200", "split-77x328x1160"],
    "split_tap_state_channel_0": ["conv-split-c128-8x8"],
    "kh_kw_swapped": ["conv-c8-9x7", "conv-c64-9x7"],
    "pad_l_for_pad_t": ["conv-c16-pad-2-1-9x7", "conv-c64-pad-2-1-9x7"],
    "odd_tstride_taps_kept": ["conv-c136-dgrad-vae-down-12x8", "conv-c48-dgrad-s2-10x6", "conv-c128-dgrad-vae-down-12x8", "conv-c64-dgrad-vae-down-12x8"],
    "ups_floor_before_sign_test": ["conv-c72-ups-5x3", "conv-c64-ups-5x3"],
    "image_bias_row_of_tile_start": ["conv-c64-b3-5x4-image-bias"],
    "residual_pitch_ldc": ["dense-130x72x200", "dense-257x136x320"],
    "geglu_pair_shifted": ["geglu-77x128x16"],
    "full_store_on_ragged_chunk": ["heads-d24", "dense-33x75x72"],
    "third_group_folded_into_second": ["gn-cg5", "gn-g6-cg5", "gn-rows100-cg5", "gn-conv-c64-b3-8x8-cg5"],
    "stats_second_image_to_first": ["gn-cg4", "gn-rows100-cg5"],
    "split_partial_left_out": ["split-128x64x1024", "split-64x64x1216"],
}
EXPECTED_FAMILY = {"residual_pitch_ldc": "poison", "geglu_pair_shifted": "pairing", "full_store_on_ragged_chunk": "sentinel",
                   "third_group_folded_into_second": "stats", "stats_second_image_to_first": "stats"}


def test_each_seeded_defect_is_caught():
    assert set(CANDIDATES) == set(gr.DEFECTS) and len(gr.DEFECTS) == 13
    print()
    for defect in gr.DEFECTS:
        for name in CANDIDATES[defect]:
            cell = gr.BY_NAME[name]
            p = probe(cell, True)
            assert gr.check(p, *gr.model(p, _splits(cell), 64)) is None
            got = gr.check(p, *gr.model(p, _splits(cell), 64, defect))
            assert got is not None, f"{defect} passes every probe of {name}"
            assert got[0] == EXPECTED_FAMILY.get(defect, "field"), (defect, got)
            print(f"    {defect:34s} caught by {got[0]:9s} {got[1]}")


def test_third_group_exists_only_at_five_channels():
    """an 8-aligned chunk of 8 columns holds columns of three groups only when a group is 5 wide (widths >= 4): why the epilogue's third
    bucket is enough, and which cells reach it"""
    three = set()
    for cg in range(4, 65):
        for n in range(0, 8 * cg * 8, 8):
            if (n + 7) // cg - n // cg >= 2:
                three.add(cg)
            assert (n + 7) // cg - n // cg <= 2
    assert three == {5}
    assert {c.name for c in gr.GN if c.N // c.gn[0] == 5 or (c.conv and c.conv.Cout // c.gn[0] == 5)} >= {"gn-cg5", "gn-split-cg5", "gn-g6-cg5"}
