"""CPU side of the VAE-encoder backward tests (tests/test_gpu_sd_vae_backward.py, tests/test_sd_vae_backward_host.py): torch on the CPU only,
nothing of the library is imported here.

Every case returns
    inputs   the tensors handed to the kernels, float32 holding values already rounded to half (biases / norm affines stay float32),
    ref64    the same operation in float64 through torch autograd: no rounding anywhere,
    emul     the same chain in float32 with a rounding to half at every tensor the product stores as half (the list below).

The one bound of the GPU tests, for every compared tensor and over ALL of its elements:

    e(x) = max|x - ref64| / max|ref64|            e(got) <= 3 * e(emul) + 2**-11

3: the kernels round where the emulation rounds but sum in another order (MFMA tiles, split-K), so at each rounding point they can land one
half-ulp step away from the emulation's correctly rounded value (1.5 ulp against 0.5 ulp).  2**-11: one half rounding of the largest element,
for tensors where the emulation happens to be exact.  e(emul) is measured against ref64, never against the kernels.

Rounding points (the tensor, and the line of the product that stores it as half)

  attention (sd/vae.py::_Attention1Head)
    S    ops.py attention_scores: `S = torch.empty(..., dtype=torch.float16)`, written by the GEMM `_launch(d, q.device)`
    P    ops.py attention_scores: `cnerf_sd_softmax_forward(ptr(S), ...)` overwrites S in place
    O    ops.py attention_apply: `O = torch.empty(B, Tq, C, dtype=torch.float16)`
    dV   vae.py backward: `ops.gemm_nt(PT, dOT, ..., dv[b])`                       (dv = torch.empty_like(v))
    dP   vae.py backward: `dP = torch.empty(T, ld, **half)`, `ops.gemm_nt(dO[b], v[b], ..., dP)`
    dS   vae.py backward: `ops.softmax_backward_(Pb, dP, T, T, ld)` overwrites dP in place
    dQ   vae.py backward: `ops.gemm_nt(dP, kT, ..., dq[b], alpha=ctx.alpha)`
    dK   vae.py backward: `ops.gemm_nt(dST, qT, ..., dk[b], alpha=ctx.alpha)`
    (the transposes PT, dOT, kT, dST, qT copy halfs: no rounding)
  linear (sd/vae.py::_Linear)
    y    ops.py linear: `out = torch.empty(M, No, dtype=torch.float16)`; bias and residual are added in float32 before the rounding
    dx   vae.py backward: `ops.linear(dy, ctx.wT)`
  convolution (sd/vae.py::_Conv)
    y    ops.py conv2d: `y = torch.empty(B, Ho, Wo, Cout, dtype=torch.float16)`; bias and residual join in float32 before the rounding
    dx   vae.py backward: `ops.conv2d(dy, ctx.wd, None, ctx.k, stride=1, pad=ctx.k - 1 - ctx.pad, tstride=ctx.stride, out_hw=ctx.in_hw)`
  GroupNorm (sd/vae.py::_GroupNorm)
    y    ops.py groupnorm: `y = torch.empty_like(x)` (normalise, affine and SiLU in float32, one rounding)
    dx   ops.py groupnorm_backward: `dx = torch.empty_like(x)`
    (the statistics are exact fixed-point sums of the half inputs: no rounding point)
  residual block (sd/vae.py::_ResnetFn), forward then backward
    h1   forward `h, s1 = ops.groupnorm(x, *blk.n1, ...)`
    c1   forward `c1, ok1 = ops.conv2d(h, c1w.w, ...)`
    h2   forward `h, _ = ops.groupnorm(c1, *blk.n2, ...)`
    res  forward `res = ops.linear(x, blk.sc.w, bias=blk.sc.b)` (blocks with a shortcut; else res is x itself)
    y    forward `y = ops.conv2d(h, c2w.w, ..., residual=res)`: the shortcut joins in float32 inside the epilogue
    d2   backward `d = ops.conv2d(dy, c2w.wd, ...)`
    dc1  backward `d = ops.groupnorm_backward(c1, d, *blk.n2, ...)`
    dh1  backward `d = ops.conv2d(d, c1w.wd, ...)`
    skip backward `skip = ops.linear(dy, blk.sc.wT)` (blocks with a shortcut; else skip is dy itself)
    dx   backward `dx = ops.groupnorm_backward(x, d, *blk.n1, ..., residual=skip)`: skip joins in float32 inside the apply kernel
  conv -> GroupNorm (the producer / consumer pair whose statistics travel three ways): y and dx of each, as listed above
"""
import functools
import math
import types

import torch
import torch.nn.functional as F

FACTOR = 3.0
FLOOR = 2.0 ** -11
GROUPS, EPS = 32, 1e-6               # the product's GroupNorm configuration (sd/arch.py VAE_SD15)


def h(t):
    """round to half precision, keep the dtype"""
    return t.half().to(t.dtype)


def err(x, ref):
    """e(x) = max|x - ref| / max|ref| over all elements (inf when x holds a non-finite value)"""
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if not bool(torch.isfinite(x).all()):
        return float("inf")
    return float((x - ref).abs().max() / ref.abs().max())


def bound(e_emul):
    return FACTOR * e_emul + FLOOR


def case(inputs, ref64, emul):
    return types.SimpleNamespace(inputs=inputs, ref64=ref64, emul=emul)


def _vjp(fn, x, dy):
    """gradient of fn at x (x's dtype) for the output gradient dy"""
    x = x.detach().clone().requires_grad_(True)
    y = fn(x)
    g, = torch.autograd.grad(y, x, dy.to(y.dtype))
    return g


# ------------------------------------------------------------------------------------------------ softmax alone
# (cols, ld): for each k_softmax<CPL> instantiation one row length with ld == cols and at least one with pad columns
SOFTMAX_SHAPES = [(8, 8), (300, 304), (1024, 1024), (513, 520), (2048, 2048), (1100, 1104), (4096, 4096), (2050, 2056), (4090, 4096)]
SOFTMAX_ROWS = (1, 5, 9)             # a workgroup holds 4 rows: one partial group, one full + 1, two full + 1


def softmax_instantiation(ld):
    """the CPL of k_softmax<CPL, *> that so_softmax (csrc/sd_ops.hip) launches for a row of ld halfs: a lane holds CPL chunks of 8 columns,
    cpl = ceil(ld / 8 / 64) chunks are needed; 1 -> <1>, 2 -> <2>, 3..4 -> <4>, 5..8 -> <8>"""
    cpl = (ld // 8 + 63) // 64
    return 1 if cpl == 1 else 2 if cpl == 2 else 4 if cpl <= 4 else 8


@functools.lru_cache(maxsize=None)
def softmax_case(rows, cols):
    """inputs S (scores, std 4 like the attention cases), P (the half probabilities the backward kernel reads), dP; results P and dS"""
    g = torch.Generator().manual_seed(7 * cols + rows)
    S = h(torch.randn(rows, cols, generator=g) * 4.0)
    dP = h(torch.randn(rows, cols, generator=g))
    P64 = torch.softmax(S.double(), -1)
    P_in = h(P64.float())

    def bwd(P, d):
        return P * (d - (P * d).sum(-1, keepdim=True))

    ref64 = dict(P=P64, dS=bwd(P_in.double(), dP.double()))
    emul = dict(P=h(torch.softmax(S, -1)), dS=h(bwd(P_in, dP)))
    return case(dict(S=S, P=P_in, dP=dP), ref64, emul)


# ------------------------------------------------------------------------------------------------ _Attention1Head
ATTENTION_SHAPES = [(1, 64, 32), (2, 99, 64), (1, 520, 64), (1, 1100, 32), (1, 2050, 16), (2, 625, 128)]      # (B, T, C)
ATTENTION_TENSORS = ("O", "dQ", "dK", "dV")
Q_SCALE = 4.0                        # logit std about 4: rows of P with a mean maximum of 0.3 .. 0.6, |S| <= 27


def attention_emul(q, k, v, dO, mutate=None):
    """float32 with the product's roundings.  mutate: None | 'alpha_dq' (alpha 2 % off in dQ only) | 'no_centring' (dS = P * dP)"""
    alpha = 1.0 / math.sqrt(q.shape[-1])
    S = h(alpha * (q @ k.transpose(1, 2)))
    P = h(torch.softmax(S, -1))
    O = h(P @ v)
    dV = h(P.transpose(1, 2) @ dO)
    dP = h(dO @ v.transpose(1, 2))
    centre = 0.0 if mutate == "no_centring" else (P * dP).sum(-1, keepdim=True)
    dS = h(P * (dP - centre))
    dQ = h((alpha * (1.02 if mutate == "alpha_dq" else 1.0)) * (dS @ k))
    dK = h(alpha * (dS.transpose(1, 2) @ q))
    return dict(O=O, dQ=dQ, dK=dK, dV=dV)


@functools.lru_cache(maxsize=None)
def attention_case(B, T, C):
    g = torch.Generator().manual_seed(1000 * B + T + C)
    q = h(torch.randn(B, T, C, generator=g) * Q_SCALE)
    k, v, dO = (h(torch.randn(B, T, C, generator=g)) for _ in range(3))
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    O64 = torch.softmax(q64 @ k64.transpose(1, 2) / math.sqrt(C), -1) @ v64
    dQ, dK, dV = torch.autograd.grad(O64, (q64, k64, v64), dO.double())
    return case(dict(q=q, k=k, v=v, dO=dO), dict(O=O64.detach(), dQ=dQ, dK=dK, dV=dV), attention_emul(q, k, v, dO))


@functools.lru_cache(maxsize=None)
def gemm_nt_case(M=99, N=52, K=72, lda=80, ldb=88, ldc=64, alpha=0.37):
    """out[M, :N] = alpha A B^T, every operand with a row stride beyond its row length (lda, ldb > K, ldc > N)"""
    g = torch.Generator().manual_seed(M + N + K)
    A, Bm = h(torch.randn(M, K, generator=g)), h(torch.randn(N, K, generator=g) / math.sqrt(K))
    return case(dict(A=A, B=Bm, alpha=alpha, lda=lda, ldb=ldb, ldc=ldc), dict(out=alpha * (A.double() @ Bm.double().t())), dict(out=h(alpha * (A @ Bm.t()))))


# ------------------------------------------------------------------------------------------------ _Linear
LINEAR_SHAPES = [(99, 64, 40), (625, 128, 128)]          # (M, K, N)


@functools.lru_cache(maxsize=None)
def linear_case(M, K, N, residual):
    g = torch.Generator().manual_seed(M + K + N)
    x, dy = h(torch.randn(M, K, generator=g)), h(torch.randn(M, N, generator=g))
    w = h(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g) * 0.1
    r = h(torch.randn(M, N, generator=g)) if residual else None

    def run(dt, rnd):
        y = x.to(dt) @ w.to(dt).t() + b.to(dt)
        if r is not None:
            y = y + r.to(dt)
        return dict(y=rnd(y), dx=rnd(dy.to(dt) @ w.to(dt)))

    return case(dict(x=x, w=w, b=b, r=r, dy=dy), run(torch.float64, lambda t: t), run(torch.float32, h))


# ------------------------------------------------------------------------------------------------ _Conv
# (kind, B, Cin, Cout, H, W, residual); kind 's1': 3 x 3, stride 1, pad 1; 'down': the VAE downsample F.pad(0, 1, 0, 1) + stride 2, out = H // 2
CONV_CASES = [("s1", 1, 64, 72, 9, 7, False), ("s1", 2, 64, 72, 9, 7, True),
              ("down", 1, 128, 128, 24, 16, False), ("down", 2, 128, 128, 24, 16, False),
              ("down", 1, 128, 128, 25, 15, False), ("down", 2, 128, 128, 25, 15, False)]


def conv_fn(kind, w, b):
    if kind == "s1":
        return lambda x: F.conv2d(x, w, b, padding=1)
    return lambda x: F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)


@functools.lru_cache(maxsize=None)
def conv_case(kind, B, Cin, Cout, H, W, residual, mutate=None):
    """mutate: None | 'drop_last_row' (an input gradient that never writes the last input row)"""
    g = torch.Generator().manual_seed(Cin + Cout + 10 * H + W + B)
    x = h(torch.randn(B, Cin, H, W, generator=g))
    w = h(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g) * 0.1
    y_shape = conv_fn(kind, w, b)(x).shape
    dy = h(torch.randn(y_shape, generator=g))
    r = h(torch.randn(y_shape, generator=g)) if residual else None

    def run(dt, rnd):
        fn = conv_fn(kind, w.to(dt), b.to(dt))
        y = fn(x.to(dt))
        if r is not None:
            y = y + r.to(dt)
        return dict(y=rnd(y), dx=rnd(_vjp(fn, x.to(dt), dy)))

    emul = run(torch.float32, h)
    if mutate == "drop_last_row":
        emul["dx"][:, :, -1, :] = 0.0
    return case(dict(x=x, w=w, b=b, r=r, dy=dy), run(torch.float64, lambda t: t), emul)


# ------------------------------------------------------------------------------------------------ conv -> _GroupNorm
def _affine(C, g):
    return 1.0 + 0.1 * torch.randn(C, generator=g), 0.02 * torch.randn(C, generator=g)


def gn_fn(gamma, beta, silu):
    if silu:
        return lambda x: F.silu(F.group_norm(x, GROUPS, gamma, beta, EPS))
    return lambda x: F.group_norm(x, GROUPS, gamma, beta, EPS)


@functools.lru_cache(maxsize=None)
def conv_gn_case(B, Cin, Cout, H, W, silu):
    """x -> c = conv3x3(x) -> y = GroupNorm(c) (+ SiLU); gradients dc (at c) and dx for the output gradient dy"""
    g = torch.Generator().manual_seed(Cin + Cout + 10 * H + W + B + int(silu))
    x = h(torch.randn(B, Cin, H, W, generator=g))
    w = h(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g) * 0.1
    gamma, beta = _affine(Cout, g)
    dy = h(torch.randn(B, Cout, H, W, generator=g))

    def run(dt, rnd):
        conv, norm = conv_fn("s1", w.to(dt), b.to(dt)), gn_fn(gamma.to(dt), beta.to(dt), silu)
        c = rnd(conv(x.to(dt)))
        y = rnd(norm(c))
        dc = rnd(_vjp(norm, c, dy))
        return dict(c=c, y=y, dc=dc, dx=rnd(_vjp(conv, x.to(dt), dc)))

    return case(dict(x=x, w=w, b=b, gamma=gamma, beta=beta, dy=dy), run(torch.float64, lambda t: t), run(torch.float32, h))


# ------------------------------------------------------------------------------------------------ _ResnetFn
def resnet_state_dict(Cin, Cout, g, p="r."):
    """diffusers' names (oracle/sd_oracle.py::resnet, sd/vae.py::_Resnet); matrices rounded to half as the product stores them"""
    sd = {}
    sd[p + "norm1.weight"], sd[p + "norm1.bias"] = _affine(Cin, g)
    sd[p + "conv1.weight"] = h(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    sd[p + "conv1.bias"] = 0.02 * torch.randn(Cout, generator=g)
    sd[p + "norm2.weight"], sd[p + "norm2.bias"] = _affine(Cout, g)
    sd[p + "conv2.weight"] = h(torch.randn(Cout, Cout, 3, 3, generator=g) / math.sqrt(9 * Cout))
    sd[p + "conv2.bias"] = 0.02 * torch.randn(Cout, generator=g)
    if Cin != Cout:
        sd[p + "conv_shortcut.weight"] = h(torch.randn(Cout, Cin, 1, 1, generator=g) / math.sqrt(Cin))
        sd[p + "conv_shortcut.bias"] = 0.02 * torch.randn(Cout, generator=g)
    return sd


def resnet_emul(x, dy, sd, p="r."):
    """the block in float32 with the roundings of _ResnetFn (module docstring)"""
    n1 = gn_fn(sd[p + "norm1.weight"], sd[p + "norm1.bias"], True)
    n2 = gn_fn(sd[p + "norm2.weight"], sd[p + "norm2.bias"], True)
    c1f = conv_fn("s1", sd[p + "conv1.weight"], sd[p + "conv1.bias"])
    c2f = conv_fn("s1", sd[p + "conv2.weight"], sd[p + "conv2.bias"])
    shortcut = (p + "conv_shortcut.weight") in sd
    h1 = h(n1(x))
    c1 = h(c1f(h1))
    h2 = h(n2(c1))
    if shortcut:
        wsc = sd[p + "conv_shortcut.weight"]
        res = h(F.conv2d(x, wsc, sd[p + "conv_shortcut.bias"]))
    else:
        res = x
    y = h(c2f(h2) + res)
    d2 = h(_vjp(c2f, h2, dy))
    dc1 = h(_vjp(n2, c1, d2))
    dh1 = h(_vjp(c1f, h1, dc1))
    skip = h(_vjp(lambda t: F.conv2d(t, wsc), x, dy)) if shortcut else dy
    dx = h(_vjp(n1, x, dh1) + skip)
    return dict(y=y, dx=dx)


@functools.lru_cache(maxsize=None)
def resnet_case(B, Cin, Cout, H, W):
    from oracle import sd_oracle as so
    g = torch.Generator().manual_seed(Cin + Cout + 10 * H + W + B)
    sd = resnet_state_dict(Cin, Cout, g)
    x = h(torch.randn(B, Cin, H, W, generator=g))
    dy = h(torch.randn(B, Cout, H, W, generator=g))
    sd64 = {k: v.double() for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    y64 = so.resnet(x64, None, sd64, "r.", GROUPS, EPS)
    dx64, = torch.autograd.grad(y64, x64, dy.double())
    return case(dict(x=x, dy=dy, sd=sd), dict(y=y64.detach(), dx=dx64), resnet_emul(x, dy, sd))


# ------------------------------------------------------------------------------------------------ whole encoder
def encoder_reference(sd, cfg, img, noise, dlat, size):
    """oracle/sd_oracle.py::encode_imgs in float32 behind the bilinear resize, as tests/test_gpu_sd_nets.py::test_vae_encode_forward_backward
    states it -> (latents, d latents / d image)"""
    from oracle import sd_oracle as so
    img = img.clone().requires_grad_(True)
    lat = so.encode_imgs(sd, cfg, F.interpolate(img, size, mode="bilinear", align_corners=False), noise)
    lat.backward(dlat)
    return lat.detach(), img.grad
