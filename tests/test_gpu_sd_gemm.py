"""GPU: the GEMM / implicit-convolution kernels of csrc/sd_gemm.hip against probes whose answer is known exactly (tests/gemm_restatement.py;
tests/test_sd_gemm_host.py shows on the CPU that the restatement is torch's float64 conv2d / autograd / matmul, that the probes meet their
exactness conditions, and that each of thirteen seeded defects fails them).  Every comparison here is `array_equal` / `torch.equal`.

Operands are small integers in fp16, alpha a power of two, bias / per-image bias / residual integers: the result is exact whatever the order of the
fp32 additions, so the MFMA order, the K-step order and split-K partials cannot matter and one wrong element shows.  Per cell, four families:
  field     the seeded integer draw (border pixels, the last ragged row of M, the last ragged columns of N, the last ragged K chunk non-zero);
            GEGLU cells carry the pairing probe instead (gate pre-activation 0 / 16, so value * gelu(gate) is exact; a shifted pair is no integer)
  poison    the same draw with NaN in the pad of lda / ldb / ldr / ld_bias_rows, in spare rows behind A, B, the residual and the per-image bias,
            and in a guard region behind a convolution's input: a read outside the problem is a NaN output
  sentinel  C / C32 / ln_out with ldc > N where the form allows, plus spare rows, pre-filled with a bit pattern that must survive outside
            [M, N] ([M, N / 2] for GEGLU); the statistics buffer with a guard image in front and behind
  stats     gn_sums against the int64 restatement bit for bit, and y bit-equal to the run without the request
Each cell runs in its padded layout (poison + sentinel, C and C32 together, then C32 alone) through the descriptor, and in its tight layout through
ops.linear / ops.conv2d / ops.gemm_nt where they reach the form.  LayerNorm-tail cell: ln_out torch.equal ops.layernorm of the same y.

Which cell reaches which kernel form (asserted per cell: split-K from cnerf_sd_gemm_workspace_bytes > 0, the loader from mode and Cin % 64):
  dense-*, heads-*            k_sd_gemm<0, ., false, GLDS>: dense LDS-DMA loader, one launch; heads-*: batch_outer x batch_inner head slices;
                              dense-33x75x72 and heads-* (N = 45) have a ragged last 8-column chunk
  split-*                     k_sd_gemm<0, ., true, GLDS> + k_sd_gemm_splitk_epilogue: the 4-column form; split-77x90: the element-wise form;
                              split-77x92: the 4-column form with residual rows 4 bytes off; split-ln-*: k_sd_gemm_splitk_epilogue_ln<4>
  conv-c8 / c40 / c72 / c48 / c24 / c16    k_sd_gemm<1, ., false>: register-staged, tap per 16-byte chunk; conv-c136-dgrad: the same, split-K
  conv-c64-9x7, -c64-s2, -c64-vae-down, -c192-1x1, -c64-b3, -c64-pad      k_sd_gemm<2, ., false, GLDS, SIMPLE>: plain-stride LDS-DMA
  conv-c64-dgrad-vae-down, conv-c64-ups    k_sd_gemm<2, ., false, GLDS, false>: general LDS-DMA form (tstride 2 / ups 2)
  conv-c128-s2, -c128-vae-down (SIMPLE), -c128-dgrad-vae-down (general)     the same loaders on the split-K schedule: K = 1152 is 18 K steps,
                              which the plan splits in two at these sizes (the Cin 64 twins are there to reach the forms in one launch)
  conv-split-c128-8x8         two splits of 9 K steps (asserted): the second starts at channel 64 of tap 4; conv-split-c320: six splits
  geglu-77x128x16, geglu-image-bias-*     the one-launch epilogue's pairing; geglu-split-*: the tail's (per-image bias in front of it)
  gn-*                        one-launch epilogue statistics; 5 channels per group (gn-cg5, gn-g6-cg5, gn-rows100-cg5, gn-conv-*): the three-bucket
                              instantiation; gn-split-*: the tail's tiled (32 groups) and untiled (6 groups; N = 30: element-wise) forms

Found by these probes on the commit that added them, and fixed with it: the one-launch epilogue added the columns of a chunk's third group to the
second (5 channels per group; gn-cg5, gn-g6-cg5, gn-rows100-cg5, gn-conv-c64 / c24 failed with 96 / 12 / 96 / 96 / 96 wrong sums), and the split-K
GEGLU tail left out the per-image bias (geglu-split-image-bias-80x128x1280: 2510 wrong outputs).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the sibling library
import gemm_restatement as gr      # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [c.name for c in gr.ALL_CELLS]
_PROBES = {}


def probe(cell, padded):
    """built once per session and shared, never modified"""
    key = (cell.name, padded)
    if key not in _PROBES:
        _PROBES[key] = gr.build(cell, padded)
    return _PROBES[key]


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


def _operands(p):
    if getattr(p, "on_device", None) is None:
        r = dev(p.r_buf)
        p.on_device = dict(A=dev(p.a_buf), B=dev(p.b_buf), R=None if r is None else r[p.r_off:], bias=dev(p.bias), br=dev(p.br_buf),
                           gamma=dev(p.ln_gamma), beta=dev(p.ln_beta))
    return p.on_device


def _descriptor(p, C, C32, gn=None, ln_out=None):
    from customnerf_amd._lib import ptr
    from customnerf_amd.sd import ops
    o = _operands(p)
    cell, c = p.cell, p.cell.conv
    d = ops._desc(o["A"], o["B"], C, p.M, p.N, p.K, p.lda, p.ldb, p.ldc, bias=o["bias"], bias_rows=o["br"], rows_per_bias_row=cell.bias_rows,
                  residual=o["R"], ldr=p.ldr, act=cell.act, alpha=cell.alpha, C32=C32)
    d.ld_bias_rows = p.ld_bias_rows
    d.batch_outer, d.batch_inner = p.batch
    d.sa_o, d.sa_i, d.sb_o, d.sb_i, d.sc_o, d.sc_i = p.strides
    if c is not None:
        Ho, Wo = c.hw_out()
        d.mode, d.Cin, d.H_in, d.W_in, d.H_out, d.W_out, d.KH, d.KW = 1, c.Cin, c.H, c.W, Ho, Wo, c.KH, c.KW
        d.stride, d.pad_t, d.pad_l, d.ups, d.tstride = c.stride, c.pad_t, c.pad_l, c.ups, c.tstride
    if gn is not None:
        d.gn_sums, d.gn_groups, d.gn_rows = ptr(gn[1:]), cell.gn[0], cell.gn[1]
    if ln_out is not None:
        d.ln_out, d.ln_gamma, d.ln_beta, d.ln_eps = ptr(ln_out), ptr(o["gamma"]), ptr(o["beta"]), 1e-5
    return d


def _assert_schedule(p, d):
    """the plan the cell was chosen for: a later change of sg_plan must fail here, not silently drop coverage"""
    from customnerf_amd._lib import lib, query_u64
    cell, c = p.cell, p.cell.conv
    need = query_u64(lib.cnerf_sd_gemm_workspace_bytes, ctypes.byref(d))
    assert (need > 0) == cell.split, f"{cell.name}: meant for the {'split-K' if cell.split else 'one-launch'} schedule, workspace {need} bytes"
    assert need % (4 * p.M * p.N) == 0
    assert cell.loader == ("dense" if c is None else "uniform" if c.Cin % 64 == 0 else "chunk")
    return need // (4 * p.M * p.N)


def _run(p, with_c=True, with_c32=False, with_gn=True, with_ln=False):
    """one launch on fresh sentinel-filled outputs -> (C, C32, gn, ln_out) device tensors (None where not requested)"""
    from customnerf_amd.sd import ops
    C0, C320, gn0 = p.outputs()
    C = dev(C0) if with_c else None
    C32 = dev(C320) if with_c32 else None
    gn = dev(gn0) if (with_gn and gn0 is not None) else None
    ln_out = dev(C0) if with_ln else None
    d = _descriptor(p, C, C32, gn, ln_out)
    _assert_schedule(p, d)
    split = ops._launch(d, _operands(p)["A"].device)
    assert split == p.cell.split
    return C, C32, gn, ln_out


def _check(p, C, C32, gn, what):
    msg = gr.check(p, host(C), host(C32), host(gn))
    assert msg is None, f"{what}: {msg[0]}: {msg[1]}"


def _tight_through_ops(p):
    """the tight layout through the Python entry that reaches the form -> y [batch, M, width] (None: only the descriptor reaches it)"""
    from customnerf_amd.sd import ops
    o, cell, c = _operands(p), p.cell, p.cell.conv
    if cell.heads is not None or cell.r_off or cell.ln or (c is None and cell.bias_rows):
        return None
    gn = None
    if cell.gn:
        sums = torch.zeros(p.M // cell.gn[1], cell.gn[0], 2, dtype=torch.int64, device="cuda")
        gn = (sums, cell.gn[0], cell.gn[1])
    R = None if o["R"] is None else o["R"].view(p.M, p.ldr)
    if c is None:
        if not (cell.bias or cell.residual or cell.gn or cell.act):
            out = torch.empty(p.M, p.N, dtype=torch.float16, device="cuda")
            return ops.gemm_nt(o["A"], o["B"], p.M, p.N, p.K, p.lda, p.ldb, p.N, out, alpha=cell.alpha)[None], None
        A, Bm = o["A"].view(-1, p.lda)[:, :p.K], o["B"].view(-1, p.ldb)[:, :p.K]                      # (strided views: linear takes the pitches)
        y = ops.linear(A, Bm, bias=o["bias"], residual=R, act=cell.act, alpha=cell.alpha, gn=gn)
    else:
        if c.pad_t != c.pad_l or c.KH != c.KW:
            return None
        Ho, Wo = c.hw_out()
        x = o["A"][:c.B * c.H * c.W * c.Cin].view(c.B, c.H, c.W, c.Cin)
        y = ops.conv2d(x, o["B"].view(p.N, p.K), o["bias"], c.KH, stride=c.stride, pad=c.pad_t, ups=c.ups, tstride=c.tstride, out_hw=(Ho, Wo),
                       bias_rows=None if o["br"] is None else o["br"].view(-1, p.ld_bias_rows), residual=R, gn=gn)
    if gn is not None:
        y, ok = y
        assert ok, f"{cell.name}: the statistics request was not admitted"
    return y.reshape(1, p.M, p.width), (gn[0] if gn is not None else None)


@pytest.mark.parametrize("cell", gr.ALL_CELLS, ids=IDS)
def test_cell(cell):
    geglu = cell.act == gr.ACT_GEGLU
    p = probe(cell, True)
    splits = _assert_schedule(p, _descriptor(p, dev(p.outputs()[0]), None))
    if cell.name == "conv-split-c128-8x8":
        assert splits == 2, "18 K steps in two splits of 9: the second starts mid-tap at channel offset 64"
    # padded layout: field + poison + sentinel (+ stats) in one launch, half and float outputs together
    C, C32, gn, ln = _run(p, with_c32=not geglu and not cell.ln, with_ln=cell.ln)
    _check(p, C, C32, gn, "padded, C and C32" if C32 is not None else "padded, C")
    if cell.ln:
        from customnerf_amd._lib import lib
        from customnerf_amd.sd import ops
        yes = ctypes.c_int(0)
        assert lib.cnerf_sd_gemm_serves_ln(ctypes.byref(_descriptor(p, C, None, None, ln)), ctypes.byref(yes)) == 0 and yes.value == 1
        o = _operands(p)
        y = C.view(-1, p.ldc)
        assert p.ldc == p.N
        assert bool((ln.view(-1, p.N)[p.M:].view(torch.int16) == int(np.int16(gr.SENT16.view(np.int16)))).all()), "ln_out rows past M were written"
        assert torch.equal(ln.view(-1, p.N)[:p.M], ops.layernorm(y[:p.M].contiguous(), o["gamma"], o["beta"], 1e-5)), "ln_out differs from ops.layernorm of the same y"
        Cn, _, _, _ = _run(p)                                               # the plain tail, no LayerNorm request: the same y
        assert torch.equal(Cn, C)
    if not geglu and not cell.ln:
        _, C32a, gna, _ = _run(p, with_c=False, with_c32=True)              # C NULL, C32 alone
        _check(p, None, C32a, gna, "padded, C32 alone")
    if cell.gn:
        Cp, _, _, _ = _run(p, with_gn=False)                                # the same y without the request
        _check(p, Cp, None, None, "padded, no statistics request")
        assert torch.equal(Cp, C), "y differs between the runs with and without the statistics request"
    # tight layout
    t = probe(cell, False)
    Ct, _, gnt, _ = _run(t)
    _check(t, Ct, None, gnt, "tight")
    got = _tight_through_ops(t)
    if got is not None:
        y, sums = got
        assert np.array_equal(host(y).astype(np.float64), t.expect), f"{cell.name}: through ops"
        if sums is not None:
            assert np.array_equal(host(sums), t.expect_sums), f"{cell.name}: statistics through ops"


def test_three_group_chunks_are_served_by_both_schedules():
    """5 channels per group: the chunk at n = 8 holds columns of groups 1, 2 and 3 (8-9, 10-14, 15).  The header serves any N % gn_groups == 0
    with N / gn_groups >= 4; sg_check, ops._attach_gn and both schedules agree (test_cell's gn-*cg5 cells compare the sums exactly)."""
    from customnerf_amd.sd import ops
    for name in ("gn-cg5", "gn-split-cg5"):
        p = probe(gr.BY_NAME[name], False)
        groups, rows = p.cell.gn
        assert p.N // groups == 5
        d = ops._desc(None, None, None, p.M, p.N, p.K, p.K, p.K, p.N)
        assert ops._attach_gn(d, (torch.zeros(p.M // rows, groups, 2, dtype=torch.int64, device="cuda"), groups, rows), p.M, p.N)


def test_invalid_statistics_requests_are_rejected_without_a_launch():
    from customnerf_amd._lib import lib
    p = probe(gr.BY_NAME["gn-cg4"], True)
    for change in (dict(gn_groups=0), dict(gn_groups=48), dict(gn_groups=64), dict(gn_rows=32), dict(gn_rows=100), dict(batch_inner=2)):
        C0, _, gn0 = p.outputs()
        C, gn = dev(C0), dev(gn0)
        d = _descriptor(p, C, None, gn)
        for k, v in change.items():
            setattr(d, k, v)
        rc = lib.cnerf_sd_gemm(ctypes.byref(d), None, 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == -1, f"{change}: status {rc}"
        assert np.array_equal(host(C).view(np.uint16), C0.view(np.uint16)) and np.array_equal(host(gn), gn0), f"{change}: an output was written"
