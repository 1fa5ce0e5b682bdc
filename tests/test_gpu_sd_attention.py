"""GPU: the fused attention kernels of csrc/sd_attn.hip (and the explicit-scores path of ops.attention) against probes whose answer is known
exactly, or to a bound that is derived and not fitted (tests/attention_restatement.py; tests/test_sd_attention_host.py shows on the CPU that
the probes are sound and that each of six seeded defects fails them).

Per (head dim, shape) cell: selector, poison and causal temptation bit-equal; uniform subsets within 1 fp16 ulp; trajectories within
tol = 2^-10 (|ref| + S) + Tk 2^-24 max|v| + 2^-24 of the float64 reference.  Head dims 40 / 64 / 80 / 160 run the LDS-DMA kernels through
ops.attention and the register-staged V^T kernels through ops.attention_vt; 8 / 32 / 48, 56, 96 and 128 run the four register-staged
row-major instantiations; 512 (one head) and 20 run the explicit-scores path, on the exact probes only.

Largest measured err / tol of the trajectory family on an MI355X (printed by test_fused_cell as "worst so far"); the arithmetic model of the
host test reaches 0.489 at the same inputs:
    LDS-DMA (ops.attention, d = 40 / 64 / 80 / 160)                         0.489
    register-staged, row-major V (ops.attention, d = 8 / 32 / 48 / 56 / 96 / 128)   0.479
    register-staged, V^T (ops.attention_vt, d = 40 / 64 / 80 / 160)          0.489
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the sibling library
import attention_restatement as ar      # noqa: E402

pytestmark = pytest.mark.gpu

CELLS = [(s, False) for s in ar.SHAPES] + [(s, True) for s in ar.CAUSAL_SHAPES]
CELL_IDS = ["x".join(map(str, s)) + ("-causal" if c else "") for s, c in CELLS]
WORST = {}                               # kernel form -> largest err / tol of the trajectory family so far


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def _operands(p):
    """-> (q, k, v) on the device, uploaded once per probe in one transfer (every part 16-byte aligned); a poison probe's k and v are the
    leading rows of its padded buffers"""
    if getattr(p, "on_device", None) is None:
        parts = [p.q, p.k if p.k_buf is None else p.k_buf, p.v if p.v_buf is None else p.v_buf]
        starts = np.cumsum([0] + [(x.size + 7) // 8 * 8 for x in parts])
        flat = np.zeros(starts[-1], np.float16)
        for x, at in zip(parts, starts):
            flat[at:at + x.size] = x.reshape(-1)
        flat = torch.from_numpy(flat).cuda()
        q, k, v = (flat[at:at + x.size].view(x.shape) for x, at in zip(parts, starts))
        Tk = p.k.shape[1]
        p.on_device = (q, k[:, :Tk], v[:, :Tk])
    return p.on_device


def _check_exact(p, fn, what):
    q, k, v = _operands(p)
    o = fn(q, k, v, p.heads, p.causal)
    msg = ar.check_exact(p, host(o))
    assert msg is None, f"{what}: {msg}"
    if p.k_buf is not None:                                                # the same bits as on the unpadded contiguous copy
        assert not k.is_contiguous() or k.shape[0] == 1
        o_c = fn(q, k.contiguous(), v.contiguous(), p.heads, p.causal)
        assert torch.equal(o, o_c), f"{what}: {p.name}: differs from the run on the contiguous copy"
    return o


def _check_trajectory(p, ref, spread, fn, form):
    o = fn(*_operands(p), p.heads, p.causal)
    r = ar.err_over_tol(host(o), ref, spread, p.v, p.k.shape[1])
    WORST[form] = max(WORST.get(form, 0.0), r)
    print(f"    {form:28s} {p.name:28s} err / tol {r:.3f}")
    assert r < 1.0, f"{form}: {p.name}: err / tol = {r:.3f}"
    return o


def _attention(q, k, v, heads, causal):
    from customnerf_amd.sd import ops
    return ops.attention(q, k, v, heads, causal)


def _attention_vt(q, k, v, heads, causal):
    from customnerf_amd.sd import ops
    return ops.attention_vt(q, k, ops.transpose_v(v), heads, causal)


def _fused_views(p):
    """q, k, v as column slices of one qkv buffer (Tq == Tk), else k and v as slices of one kv buffer"""
    q, k, v = _operands(p)
    C = q.shape[2]
    if q.shape[1] == k.shape[1]:
        qkv = torch.cat([q, k, v], -1)
        return qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    kv = torch.cat([k, v], -1)
    return q, kv[..., :C], kv[..., C:]


@pytest.mark.parametrize("shape,causal", CELLS, ids=CELL_IDS)
@pytest.mark.parametrize("d", ar.FUSED_DIMS)
def test_fused_cell(d, shape, causal):
    B, heads, Tq, Tk = shape
    dma = d in ar.DMA_DIMS
    form = "LDS-DMA" if dma else "register-staged row-major V"
    exact = ar.exact_probes(B, heads, Tq, Tk, d, causal)
    traj = ar.trajectory_probes(B, heads, Tq, Tk, d, causal)
    print(f"[d {d}, {'x'.join(map(str, shape))}{' causal' if causal else ''}]")
    outs = {}
    for p in exact:
        outs[p.name] = _check_exact(p, _attention, form)
    refs = dict(zip((p.name for p in traj), ar.references(traj)))
    for p in traj:
        outs[p.name] = _check_trajectory(p, *refs[p.name], _attention, form)
    if dma:                                                                # the pre-transposed-V entry: the register-staged kernels, VROW = false
        for p in exact:
            o = _check_exact(p, _attention_vt, "register-staged V^T")
            if p.name.startswith("selector"):
                assert torch.equal(o, outs[p.name]), f"attention and attention_vt differ on {p.name}"
        for p in traj:
            o = _check_trajectory(p, *refs[p.name], _attention_vt, "register-staged V^T")
            assert torch.equal(o, outs[p.name]), f"attention and attention_vt differ on {p.name}"
    for p in (exact[0], traj[0]):                                          # strided views of a fused projection: the same bits
        q, k, v = _fused_views(p)
        assert not k.is_contiguous() or k.shape[:2] == (1, 1)
        assert torch.equal(_attention(q, k, v, heads, causal), outs[p.name]), f"{form}: fused-buffer views differ on {p.name}"
    print("    worst so far: " + ", ".join(f"{f} {r:.3f}" for f, r in WORST.items()))


@pytest.mark.parametrize("shape", ar.SHAPES, ids=CELL_IDS[:len(ar.SHAPES)])
@pytest.mark.parametrize("d,one_head", [(512, True), (20, False)])
def test_explicit_scores_cell(d, one_head, shape):
    """d > 160 and d % 8 != 0: attention_scores -> softmax -> attention_apply, with amplitudes its fp16 scores hold"""
    B, heads, Tq, Tk = shape
    heads = 1 if one_head else heads
    for p in ar.exact_probes(B, heads, Tq, Tk, d, False, "f16"):
        _check_exact(p, _attention, f"explicit scores, d = {d}")


# ---------------------------------------------------------------------------------------------------------------- the C entry points
SENTINEL = -1234.0
CANARY = (2, 2, 33, 65)                   # B, heads, Tq, Tk


def _abi_args(d, vt, pad_cols=8, pad_rows=3):
    """a selector probe and the argument list of cnerf_sd_attention_v (vt False) / cnerf_sd_attention (vt True), out with spare rows and columns"""
    from customnerf_amd._lib import ptr, stream
    from customnerf_amd.sd import ops
    B, heads, Tq, Tk = CANARY
    p = ar.selector("perm", B, heads, Tq, Tk, d)
    C = heads * d
    q, k, v = dev(p.q), dev(p.k), dev(p.v)
    ldo = C + pad_cols
    out = torch.full((B, Tq + pad_rows, ldo), SENTINEL, dtype=torch.float16, device="cuda")
    if vt:
        v = ops.transpose_v(v)
        ldv, sv = v.shape[2], C * v.shape[2]
    else:
        ldv, sv = C, Tk * C
    args = dict(q=ptr(q), k=ptr(k), v=ptr(v), out=ptr(out), B=B, H=heads, Tq=Tq, Tk=Tk, d=d, ldq=C, sq=Tq * C, ldk=C, sk=Tk * C, ldv=ldv, sv=sv,
                ldo=ldo, so=(Tq + pad_rows) * ldo, causal=0, stream=stream())
    return p, args, out, (q, k, v)


def _call(vt, args):
    from customnerf_amd._lib import lib
    fn = lib.cnerf_sd_attention if vt else lib.cnerf_sd_attention_v
    return fn(*[args[n] for n in ("q", "k", "v", "out", "B", "H", "Tq", "Tk", "d", "ldq", "sq", "ldk", "sk", "ldv", "sv", "ldo", "so", "causal", "stream")])


@pytest.mark.parametrize("vt", [False, True], ids=["row_major_v", "v_transposed"])
@pytest.mark.parametrize("d", ar.FUSED_DIMS)
def test_output_canary(d, vt):
    """rows >= Tq and columns >= heads * d of the output buffer are not written"""
    from customnerf_amd._lib import check
    p, args, out, keep = _abi_args(d, vt)
    check(_call(vt, args), "sd_attention")
    torch.cuda.synchronize()
    B, heads, Tq, Tk = CANARY
    o = host(out)
    assert (o[:, Tq:] == np.float16(SENTINEL)).all(), "rows past Tq were written"
    assert (o[:, :, heads * d:] == np.float16(SENTINEL)).all(), "columns past heads * d were written"
    assert (o[:, :Tq, :heads * d].view(np.uint16) == p.expect.view(np.uint16)).all()


BAD_ARGS = [("d_zero", dict(d=0)), ("d_12", dict(d=12)), ("d_168", dict(d=168)), ("tq_zero", dict(Tq=0)),
            ("ldq", dict(ldq=+4)), ("ldk", dict(ldk=+4)), ("ldv", dict(ldv=+4)), ("ldo", dict(ldo=+2)), ("ldv_short", dict(ldv=-32)),
            ("null_q", dict(q=None)), ("null_k", dict(k=None)), ("null_v", dict(v=None)), ("null_out", dict(out=None)), ("q_plus_8_bytes", dict(q=+8))]


# ldv >= round32(Tk) is a rule of the V^T entry only
BAD_CALLS = [(n, c, vt) for vt in (False, True) for n, c in BAD_ARGS if vt or n != "ldv_short"]


@pytest.mark.parametrize("name,change,vt", BAD_CALLS, ids=[f"{n}-{'v_transposed' if vt else 'row_major_v'}" for n, _, vt in BAD_CALLS])
def test_invalid_arguments_are_rejected_without_a_launch(name, change, vt):
    """at_launch's rules: a negative status, and the output buffer keeps its sentinel"""
    p, args, out, keep = _abi_args(64, vt, pad_cols=0, pad_rows=0)
    if name == "ldv" and vt:
        change = dict(ldv=+2)                                              # V^T rows are read in 8-byte halves: ldv % 4
    for key, val in change.items():
        if val is None or key in ("d", "Tq"):
            args[key] = val
        else:
            args[key] = args[key] + val                                    # a pitch or a pointer moved off its alignment, ldv below round32(Tk)
    rc = _call(vt, args)
    torch.cuda.synchronize()
    assert rc < 0, f"{name}: status {rc}"
    assert rc == (-2 if name.startswith("null") else -1)
    assert bool((out == SENTINEL).all()), f"{name}: the output buffer was written"
