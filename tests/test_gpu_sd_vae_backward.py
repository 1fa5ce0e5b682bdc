"""GPU: every hand-written backward of the VAE encoder (customnerf_amd/sd/vae.py: _Conv, _GroupNorm, _Linear, _Attention1Head, _ResnetFn, and the
whole encoder at a ragged size) against float64 autograd, at the shapes the product's 512 x 512 run never takes: token counts with pad columns
(ld = pad8(T) != T), B > 1, odd image sizes under the stride-2 downsample, every k_softmax<CPL> instantiation, and each of the three ways a
GroupNorm gets its statistics (the producing GEMM's epilogue, the split-K tail, the norm itself).

One bound for every compared tensor, over all of its elements (tests/vae_backward_testlib.py):

    e(x) = max|x - ref64| / max|ref64|            e(got) <= 3 * e(emul) + 2**-11

with e(emul) the error of a float32 emulation that rounds to half where the product stores a half, measured in the same run against the same
float64 reference.  tests/test_sd_vae_backward_host.py shows on the CPU that a 2 % error in one term breaks this bound.

Measured on the MI355X, ratio e(got) / e(emul) per tensor (e(emul) itself in brackets); the factor 3 was never needed, nothing was raised:
    softmax alone, 9 row lengths x 3 row counts      P 1.00, dS 1.00 at every shape                         (0.6e-4 .. 4.5e-4)
    attention, all six shapes                        O 1.00 (1.4e-3 .. 2.6e-3), dQ 1.00 (1.3e-3 .. 3.0e-3), dK 1.00 (1.6e-3 .. 2.4e-3),
                                                     dV 1.00 (0.8e-3 .. 1.8e-3)
    gemm_nt 99x52x72, lda 80, ldb 88, ldc 64         out 1.00                                               (3.2e-4)
    linear 99x64->40, 625x128->128, +- residual      y 1.00, dx 1.00                                        (2.6e-4 .. 3.8e-4)
    conv 3x3 64->72 at 9x7; downsample at 24x16,     y 1.00, dx 1.00, last input row / column of dx 1.00    (2.4e-4 .. 4.0e-4)
      25x15, B 1 and 2
    conv + GroupNorm, statistics from the epilogue   c, y, dc, dx 1.00                                      (3.4e-4 .. 5.2e-4)
      from the split-K tail                          c, y, dc, dx 1.00                                      (2.4e-4 .. 4.6e-4)
      by the norm itself (35 rows)                   c, y, dc 1.00, dx 1.00 .. 1.04                         (2.8e-4 .. 5.1e-4)
    resnet 128->128 / 128->256 at 9x8 (tail)         y 1.00, dx 1.00 .. 1.01                                (2.9e-4 .. 5.7e-4)
    resnet at 5x7 (self), 128->256 at 33x31          y 1.00, dx 1.00                                        (4.0e-4 .. 5.8e-4)
      (epilogue); out_gn and x_sums change nothing
    encoder tiny 200x136, B 2, against the oracle    latents 0.9e-3 max / 0.7e-3 L2, d image 1.6e-3 .. 1.8e-3 max / 1.7e-3 .. 1.9e-3 L2
      each image in the batch against its own run    latents 0.8e-3 .. 0.9e-3 / 0.7e-3, d image 1.8e-3 .. 1.9e-3 / 1.8e-3 .. 1.9e-3
A ratio of 1.00 means the largest error sits at an element where kernel and emulation round the same way: the float32 accumulation order moves
a value by far less than half a half-ulp, so the two disagree only at rare ties, never at the element that sets the maximum.
"""
import contextlib
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # sibling test modules' helpers
import vae_backward_testlib as tl      # noqa: E402

G, EPS = tl.GROUPS, tl.EPS
NAN = float("nan")


def dev(t):
    return t.half().cuda()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().half().cuda()


def nchw(y):
    return y.detach().permute(0, 3, 1, 2)


def compare(tag, c, got, ref=None, emul=None):
    """print e(got), e(emul) and their ratio for every tensor of `got`, then assert the bound for all of them"""
    bad = []
    for name, value in got.items():
        r = (ref or c.ref64)[name]
        value = value.detach().double().cpu()
        eg, ee = tl.err(value, r), tl.err((emul or c.emul)[name], r)
        print(f"[{tag}] {name}: e(got) {eg:.3e}  e(emul) {ee:.3e}  ratio {eg / ee if ee > 0 else float('inf'):.2f}  bound {tl.bound(ee):.3e}")
        if not eg <= tl.bound(ee):
            d = (value - r.double()).abs().nan_to_num(float("inf"))
            worst = tuple(int(i) for i in torch.unravel_index(d.argmax(), d.shape))
            bad.append(f"{name}: e(got) {eg:.3e} > 3 * {ee:.3e} + 2**-11, worst element at {worst} of {tuple(d.shape)}")
    assert not bad, f"[{tag}] " + "; ".join(bad)


@contextlib.contextmanager
def statistics_spy():
    """Which way each GroupNorm got its statistics.  log.gemm: per GEMM launch (an admissible statistics request was attached, the library ran it
    split-K); log.norm: per forward norm 'ready' (only the apply pass ran, on sums its producer delivered) or 'own' (the norm summed itself)."""
    from customnerf_amd.sd import ops
    log = types.SimpleNamespace(gemm=[], norm=[])
    launch, groupnorm = ops._launch, ops.groupnorm

    def spy_launch(d, device):
        split = launch(d, device)
        log.gemm.append((bool(d.gn_sums), bool(split)))
        return split

    def spy_groupnorm(x, gamma, beta, groups, eps, silu, pool=None, sums=None, sums_ready=True):
        log.norm.append("ready" if sums is not None and sums_ready else "own")
        return groupnorm(x, gamma, beta, groups, eps, silu, pool=pool, sums=sums, sums_ready=sums_ready)

    ops._launch, ops.groupnorm = spy_launch, spy_groupnorm
    try:
        yield log
    finally:
        ops._launch, ops.groupnorm = launch, groupnorm


def statistics_path(gemm_entry, norm_entry):
    requested, split = gemm_entry
    if not requested:
        assert norm_entry == "own", "no statistics were requested from the producer, yet the norm did not compute its own"
        return "self"
    assert norm_entry == "ready", "the producer delivered statistics, yet the norm summed again"
    return "tail" if split else "epilogue"


def assert_sums_match(sums, y_nhwc, tag):
    """delivered fixed-point statistics against the exact sums of the half tensor they describe"""
    from customnerf_amd.sd import ops
    B, C = y_nhwc.shape[0], y_nhwc.shape[-1]
    v = y_nhwc.detach().double().reshape(B, -1, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    exact = torch.stack([v.sum(-1), v.square().sum(-1)], -1)
    got = ops.gn_sums_to_float(sums)
    n = v.shape[-1]
    assert float((got - exact).abs().max()) <= 1e-4 * n, (tag, float((got - exact).abs().max()), n)     # 1e-4 per element: tests/test_gpu_sd_ops.py's mean check


# ------------------------------------------------------------------------------------------------ 1. softmax forward and backward, alone
# The instantiation each row length runs, derived from so_softmax's rule (csrc/sd_ops.hip): a lane holds CPL chunks of 8 halfs and
# cpl = ceil(ld / 8 / 64) are needed; cpl 1 -> k_softmax<1>, 2 -> <2>, 3..4 -> <4>, 5..8 -> <8>.
#   ld    8: 1 chunk    -> <1>      ld  304: 38 chunks   -> <1>
#   ld 1024: 128 chunks -> <2>      ld  520: 65 chunks   -> <2>
#   ld 2048: 256 chunks -> <4>      ld 1104: 138 chunks  -> cpl 3 -> <4>
#   ld 4096: 512 chunks -> <8>      ld 2056: 257 chunks  -> cpl 5 -> <8>
SOFTMAX_INSTANTIATION = {(8, 8): 1, (300, 304): 1, (1024, 1024): 2, (513, 520): 2, (2048, 2048): 4, (1100, 1104): 4, (4096, 4096): 8, (2050, 2056): 8,
                         (4090, 4096): 8}


def test_softmax_cases_run_every_instantiation_forward_and_backward():
    assert set(SOFTMAX_INSTANTIATION) == set(tl.SOFTMAX_SHAPES)
    for (cols, ld), cpl in SOFTMAX_INSTANTIATION.items():
        assert tl.softmax_instantiation(ld) == cpl, (cols, ld)
    assert {(cpl, ld != cols) for (cols, ld), cpl in SOFTMAX_INSTANTIATION.items()} == {(c, p) for c in (1, 2, 4, 8) for p in (False, True)}


@pytest.mark.parametrize("cols,ld", tl.SOFTMAX_SHAPES)
def test_softmax_forward_backward_alone(cols, ld):
    from customnerf_amd._lib import lib, check, ptr, stream
    from customnerf_amd.sd import ops
    cpl = SOFTMAX_INSTANTIATION[(cols, ld)]
    GUARD = 4                                   # rows behind the last one (a workgroup holds 4 rows): must stay untouched
    for rows in tl.SOFTMAX_ROWS:
        c = tl.softmax_case(rows, cols)
        tag = f"softmax<{cpl}> {rows}x{cols}/{ld}"

        def buffer(src, pad):
            t = torch.full((rows + GUARD, ld), 3.0, dtype=torch.float16, device="cuda")
            t[:rows] = pad
            t[:rows, :cols] = dev(src)
            return t

        res = {}
        for pad in (0.0, NAN):                   # the pad columns of S and dP: zeros, then NaN
            S = buffer(c.inputs["S"], pad)
            check(lib.cnerf_sd_softmax_forward(ptr(S), rows, cols, ld, stream()), "sd_softmax_forward")
            P = buffer(c.inputs["P"], 0.0)        # (the forward leaves P's pad columns zero)
            dP = buffer(c.inputs["dP"], pad)
            ops.softmax_backward_(P, dP, rows, cols, ld)
            for name, t in (("P", S), ("dS", dP)):
                assert torch.all(t[:rows, cols:] == 0), f"[{tag}] {name}: pad columns not exactly zero (pad input {pad})"
                assert torch.all(t[rows:] == 3.0), f"[{tag}] {name}: rows behind the last one were written"
            assert torch.equal(P[:rows, :cols], dev(c.inputs["P"])), f"[{tag}] the backward changed P"
            res[pad == 0.0] = dict(P=S[:rows, :cols].clone(), dS=dP[:rows, :cols].clone())
        for name in ("P", "dS"):
            assert torch.equal(res[True][name], res[False][name]), f"[{tag}] {name}: NaN in the pad columns changed the row results"
        compare(tag, c, res[False])


# ------------------------------------------------------------------------------------------------ 2. _Attention1Head
def run_attention(c):
    from customnerf_amd.sd import vae
    q, k, v = (dev(c.inputs[n]).requires_grad_(True) for n in ("q", "k", "v"))
    O = vae._Attention1Head.apply(q, k, v)
    O.backward(dev(c.inputs["dO"]))
    return dict(O=O.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)


@pytest.mark.parametrize("B,T,C", tl.ATTENTION_SHAPES)
def test_attention_one_head_forward_backward(B, T, C):
    c = tl.attention_case(B, T, C)
    ld = (T + 7) // 8 * 8
    compare(f"attention {B}x{T}x{C} ld {ld} softmax<{tl.softmax_instantiation(ld)}>", c, run_attention(c))


def test_gemm_nt_alpha_and_row_stride_beyond_n():
    from customnerf_amd.sd import ops
    c = tl.gemm_nt_case()
    i = c.inputs
    alpha, lda, ldb, ldc = i["alpha"], i["lda"], i["ldb"], i["ldc"]
    (M, K), N = i["A"].shape, i["B"].shape[0]
    assert alpha != 1.0 and lda > K and ldb > K and ldc > N

    def strided(src, ld):                       # rows of `ld` halfs, NaN behind the K the GEMM may read
        t = torch.full((src.shape[0] + 1, ld), NAN, dtype=torch.float16, device="cuda")
        t[:-1, :K] = dev(src)
        return t

    A, Bm = strided(i["A"], lda), strided(i["B"], ldb)
    out = torch.full((M + 1, ldc), 7.0, dtype=torch.float16, device="cuda")
    ops.gemm_nt(A, Bm, M, N, K, lda, ldb, ldc, out, alpha=alpha)
    assert torch.all(out[:M, N:] == 7.0), "gemm_nt wrote columns beyond N"
    assert torch.all(out[M:] == 7.0), "gemm_nt wrote rows beyond M"
    compare(f"gemm_nt {M}x{N}x{K} lda {lda} ldb {ldb} ldc {ldc} alpha {alpha}", c, dict(out=out[:M, :N]))


# ------------------------------------------------------------------------------------------------ 3. _Linear
@pytest.mark.parametrize("M,K,N", tl.LINEAR_SHAPES)
@pytest.mark.parametrize("residual", [False, True])
def test_linear_forward_backward(M, K, N, residual):
    from customnerf_amd.sd import pack, vae
    c = tl.linear_case(M, K, N, residual)
    i = c.inputs
    x = dev(i["x"]).requires_grad_(True)
    r = dev(i["r"]).requires_grad_(True) if residual else None
    w = i["w"].cuda()
    y = vae._Linear.apply(x, pack.pack_linear(w), pack.pack_linear_T(w), pack.f32(i["b"].cuda()), r)
    dy = dev(i["dy"])
    y.backward(dy)
    compare(f"linear {M}x{K}->{N} residual {residual}", c, dict(y=y, dx=x.grad))
    if residual:
        assert torch.equal(r.grad, dy), "the residual's gradient is dy itself"


# ------------------------------------------------------------------------------------------------ 4. _Conv
@pytest.mark.parametrize("kind,B,Cin,Cout,H,W,residual", tl.CONV_CASES)
def test_conv_forward_and_input_gradient(kind, B, Cin, Cout, H, W, residual):
    from customnerf_amd.sd import pack, vae
    c = tl.conv_case(kind, B, Cin, Cout, H, W, residual)
    i = c.inputs
    x = nhwc(i["x"]).requires_grad_(True)
    r = nhwc(i["r"]).requires_grad_(True) if residual else None
    w = i["w"].cuda()
    stride, pad, out_hw = (1, 1, None) if kind == "s1" else (2, 0, (H // 2, W // 2))
    y = vae._Conv.apply(x, pack.pack_conv(w), pack.pack_conv_dgrad(w), pack.f32(i["b"].cuda()), 3, stride, pad, out_hw, r, None, 0)[0]
    dy = nhwc(i["dy"])
    y.backward(dy)
    tag = f"conv {kind} {B}x{Cin}->{Cout} {H}x{W} residual {residual}"
    dx = nchw(x.grad)
    compare(tag, c, dict(y=nchw(y), dx=dx))
    if residual:
        assert torch.equal(r.grad, dy), "the residual's gradient is dy itself"
    if kind == "down":
        # the edge the padded, strided window reaches last, compared on its own: the last input row takes part in one output row only (through
        # one (H even: two) kernel rows), and the same for the last column
        edges = {"last input row": (slice(None), slice(None), slice(H - 1, H)), "last input column": (slice(None), slice(None), slice(None), slice(W - 1, W))}
        for name, sl in edges.items():
            compare(f"{tag}, {name} of dx", c, {"dx": dx[sl]}, ref={"dx": c.ref64["dx"][sl]}, emul={"dx": c.emul["dx"][sl]})


# ------------------------------------------------------------------------------------------------ 5. _GroupNorm behind a _Conv, and _ResnetFn
# (B, Cin, Cout, H, W) -> the way the norm gets its statistics.  The path follows from the GEMM's plan (sg_plan, csrc/sd_gemm.hip) and is asserted:
#   64 -> 128 at 9 x 8: K = 576 is 9 K steps, below the 16 a split needs; 72 rows per image -> the one-launch epilogue sums, its 128-row tile
#                       crossing the image boundary
#   256 -> 128 at 9 x 8: K = 2304, 144 rows: split-K -> the tail kernel sums
#   64 -> 128 at 5 x 7: 35 rows per image < 64: the request is inadmissible, the norm sums itself
CONV_GN_CASES = [(2, 64, 128, 9, 8, "epilogue"), (2, 256, 128, 9, 8, "tail"), (2, 64, 128, 5, 7, "self")]


@pytest.mark.parametrize("B,Cin,Cout,H,W,path", CONV_GN_CASES)
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_behind_conv_each_statistics_path(B, Cin, Cout, H, W, path, silu):
    from customnerf_amd.sd import ops, pack, vae
    c = tl.conv_gn_case(B, Cin, Cout, H, W, silu)
    i = c.inputs
    w = i["w"].cuda()
    wp, wd, b = pack.pack_conv(w), pack.pack_conv_dgrad(w), pack.f32(i["b"].cuda())
    gamma, beta = pack.f32(i["gamma"].cuda()), pack.f32(i["beta"].cuda())
    dy = nhwc(i["dy"])
    tag = f"conv {Cin}->{Cout} {B}x{H}x{W} + GroupNorm silu {silu}"
    x = nhwc(i["x"]).requires_grad_(True)
    sums = ops.SumsPool(1, B, G, x.device).take()
    with statistics_spy() as log:
        cv, flag = vae._Conv.apply(x, wp, wd, b, 3, 1, 1, None, None, sums, G)
        cv.retain_grad()
        y = vae._GroupNorm.apply(cv, gamma, beta, G, EPS, silu, sums, bool(flag))
    assert statistics_path(log.gemm[0], log.norm[0]) == path, (log.gemm, log.norm, bool(flag))
    assert bool(flag) == (path != "self")
    assert_sums_match(sums, cv, tag)                   # whoever summed: the buffer now holds the statistics of the conv's half output
    y.backward(dy)
    compare(f"{tag}, statistics: {path}", c, dict(c=nchw(cv), y=nchw(y), dc=nchw(cv.grad), dx=nchw(x.grad)))
    # the norm without any buffer handed in (sums_in None: it zeroes and fills its own)
    c2 = cv.detach().clone().requires_grad_(True)
    y2 = vae._GroupNorm.apply(c2, gamma, beta, G, EPS, silu)
    y2.backward(dy)
    ref = dict(y=c.ref64["y"], dc=c.ref64["dc"])
    compare(f"{tag}, statistics: none handed in", c, dict(y=nchw(y2), dc=nchw(c2.grad)), ref=ref)


# (B, Cin, Cout, H, W) -> how norm2 gets its statistics from conv1 (asserted):
#   9 x 8: 144 rows, K = 1152 (18 K steps): the plan splits K in two -> the split-K tail sums (not the epilogue: a one-launch schedule
#          needs 64 or more 128 x 64 tiles at this K)
#   5 x 7: 35 rows per image < 64 -> inadmissible, norm2 sums itself
#   33 x 31 (128 -> 256): 2046 rows x 256 columns = 64 tiles, one launch -> conv1's epilogue sums, tiles crossing the image boundary at row 1023
RESNET_CASES = [(2, 128, 128, 9, 8, "tail"), (2, 128, 256, 9, 8, "tail"), (2, 128, 128, 5, 7, "self"), (2, 128, 256, 5, 7, "self"), (2, 128, 256, 33, 31, "epilogue")]


@pytest.mark.parametrize("B,Cin,Cout,H,W,path", RESNET_CASES)
def test_resnet_block_forward_backward_each_statistics_path(B, Cin, Cout, H, W, path):
    from customnerf_amd.sd import ops, vae
    c = tl.resnet_case(B, Cin, Cout, H, W)
    i = c.inputs
    blk = vae._Resnet(i["sd"], "r.", "cuda")
    dy = nhwc(i["dy"])
    shortcut = Cin != Cout
    doubled = False
    for out_gn in (True, False):
        for x_ready in (False, True):
            tag = f"resnet {Cin}->{Cout} {B}x{H}x{W} norm2 statistics: {path}, out_gn {out_gn}, x_sums {'ready' if x_ready else 'None'}"
            x = nhwc(i["x"]).requires_grad_(True)
            pool = ops.SumsPool(8, B, G, x.device)
            x_sums = (ops.groupnorm(x.detach(), *blk.n1, G, EPS, True)[1], True) if x_ready else None
            with statistics_spy() as log:
                y, gn_out = blk(x, G, EPS, pool, x_sums=x_sums, out_gn=out_gn)
            assert len(log.norm) == 2 and len(log.gemm) == (3 if shortcut else 2), (log.norm, log.gemm)
            assert log.norm[0] == ("ready" if x_ready else "own")
            assert statistics_path(log.gemm[0], log.norm[1]) == path, (log.gemm, log.norm)
            if out_gn:
                so, ready = gn_out
                assert log.gemm[-1][0] == ready == (H * W >= 64), (log.gemm, ready)
                if ready:
                    assert_sums_match(so, y, tag)
                else:
                    assert not so.any(), "an inadmissible request must leave the pre-zeroed buffer untouched for the consumer"
            else:
                assert gn_out is None and log.gemm[-1][0] is False
            second = not doubled and out_gn and not x_ready
            y.backward(dy, retain_graph=second)
            compare(tag, c, dict(y=nchw(y), dx=nchw(x.grad)))
            if second:                                 # the pooled scratch statistics were consumed by the first pass and must not be reused
                g1 = x.grad.clone()
                y.backward(dy)
                assert torch.equal(x.grad, 2 * g1), f"[{tag}] a second backward through the retained graph is not exactly twice the first"
                doubled = True
    assert doubled


# ------------------------------------------------------------------------------------------------ 6. whole encoder, ragged
ENC_SIZE = (200, 136)                  # mid-block 25 x 17 = 425 tokens, ld 432; levels 200 x 136, 100 x 68, 50 x 34, 25 x 17


@pytest.fixture(scope="module")
def encoder_setup():
    from customnerf_amd.sd import arch
    from test_gpu_sd_nets import half_sd
    cfg = arch.VAE_TINY
    sd = half_sd(arch.random_state_dict(arch.vae_encoder_params(cfg), seed=5))
    g = torch.Generator().manual_seed(200136)
    img = torch.rand(2, 3, 48, 40, generator=g)
    noise = torch.randn(2, 4, ENC_SIZE[0] // 8, ENC_SIZE[1] // 8, generator=g)
    dlat = torch.randn(2, 4, ENC_SIZE[0] // 8, ENC_SIZE[1] // 8, generator=g)
    lat_ref, grad_ref = tl.encoder_reference(sd, cfg, img, noise, dlat, ENC_SIZE)
    return types.SimpleNamespace(cfg=cfg, sd=sd, img=img, noise=noise, dlat=dlat, lat_ref=lat_ref, grad_ref=grad_ref)


def run_encoder(s, sel=slice(None)):
    from customnerf_amd.sd.vae import VAEEncoder
    enc = VAEEncoder(s.cfg, s.sd, "cuda")
    img = s.img[sel].cuda().requires_grad_(True)
    lat = enc.encode_imgs(img, s.noise[sel].cuda(), resize=ENC_SIZE)
    lat.backward(s.dlat[sel].cuda())
    return lat.detach(), img.grad


def test_encoder_ragged_batch_of_two(encoder_setup):
    from test_gpu_sd_nets import rel_err
    s = encoder_setup
    lat, grad = run_encoder(s)
    assert lat.shape == s.lat_ref.shape == (2, 4, 25, 17) and lat.dtype == torch.float32

    def check(tag, lat_a, lat_b, grad_a, grad_b):
        emax, el2 = rel_err(lat_a, lat_b)
        gmax, gl2 = rel_err(grad_a, grad_b)
        print(f"[vae tiny {ENC_SIZE[0]}x{ENC_SIZE[1]} {tag}] latents max rel {emax:.3e}, L2 rel {el2:.3e}; d latents / d image max rel {gmax:.3e}, L2 rel {gl2:.3e}")
        # the bounds of tests/test_gpu_sd_nets.py::test_vae_encode_forward_backward
        assert emax < 5e-3 and el2 < 3e-3, (tag, "latents", emax, el2)
        assert gmax < 7.5e-3 and gl2 < 6e-3, (tag, "d latents / d image", gmax, gl2)

    check("batch vs oracle", lat, s.lat_ref, grad, s.grad_ref)
    for b in range(2):
        check(f"image {b} vs oracle", lat[b], s.lat_ref[b], grad[b], s.grad_ref[b])
        lat1, grad1 = run_encoder(s, slice(b, b + 1))
        check(f"image {b} in the batch vs alone", lat[b:b + 1], lat1, grad[b:b + 1], grad1)


# ------------------------------------------------------------------------------------------------ 7. recycled memory
def test_attention_and_ragged_encoder_are_independent_of_recycled_memory(encoder_setup):
    """PT, dOT, dP, kT, dST and qT of _Attention1Head.backward are torch.empty buffers with pad columns / rows; the ragged encoder adds the
    conv and norm workspaces at odd sizes.  One clean pass, one pass on pools filled with 0xFF (NaN as half): the same bits, no NaN."""
    from test_gpu_uninitialised import poison_allocator

    def one_pass():
        out = {}
        for B, T, C in tl.ATTENTION_SHAPES:
            for name, t in run_attention(tl.attention_case(B, T, C)).items():
                out[f"attention {B}x{T}x{C} {name}"] = t.cpu()
        lat, grad = run_encoder(encoder_setup)
        out["encoder latents"], out["encoder d image"] = lat.cpu(), grad.cpu()
        return out

    clean = one_pass()                 # (kept on the CPU: no live device tensor whose segment could hand the second pass the first pass's bytes)
    poison_allocator(1.0)
    probe = torch.empty(2056, 2056, dtype=torch.float16, device="cuda")          # the size of P^T at T = 2050
    print(f"[recycled memory] NaN fraction of a fresh torch.empty of that size: {float(torch.isnan(probe).float().mean()):.3f}")
    del probe
    dirty = one_pass()
    for name, t in clean.items():
        assert bool(torch.isfinite(dirty[name].float()).all()), f"{name}: non-finite on recycled memory"
        assert torch.equal(t, dirty[name]), f"{name}: depends on the contents of recycled memory"
