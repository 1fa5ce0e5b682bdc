"""The contract of cnerf_sd_gemm (include/customnerf_sd.h, "cnerf_sd_gemm") restated in int64 / float64 numpy, probes of it whose answer is known
exactly, and a small structural model of a kernel of this design with seeded defects.  numpy only; shared by tests/test_sd_gemm_host.py (CPU: the
restatement is right, the probes are sound and have teeth) and tests/test_gpu_sd_gemm.py (GPU: csrc/sd_gemm.hip against the probes).

Why exact: every operand is a small integer held in fp16, alpha a power of two, bias / per-image bias / residual integers.  Then every product is
exact, every fp32 partial sum of them is an integer below 2^24 whatever the order of the additions (so the MFMA order, the K-step order and the
split-K partials cannot matter), the epilogue adds exact values, and the result is an fp16 number.  The kernel's output must equal the reference
bit for bit (`array_equal`), and a single wrong element anywhere — a border tap, a ragged chunk, a column of the wrong group — shows.  The
builders assert these conditions on the reference alone (`_assert_exact`); a probe that violates one fails loudly.

Probe = a Cell (what to compute) laid out in buffers, in one of two forms:
  tight   the pitches the cell names (K / N where it names none), nothing around the operands;
  padded  every pitch the cell leaves open widened, spare rows behind A, B, the residual and the per-image bias, a guard region behind a
          convolution's input — all of it NaN (one read outside the problem turns an output into NaN: the POISON family) — and outputs with
          ldc > N plus spare rows, pre-filled with a sentinel bit pattern that must survive (the SENTINEL family); the statistics buffer
          carries one guard image in front and one behind.
`check` names the family that fails: sentinel, poison, field (pairing for GEGLU cells), stats.
"""
import math
import zlib
from dataclasses import dataclass, field

import numpy as np

FRAC_BITS = 20                           # CNERF_SD_GN_FRAC_BITS
SENT16 = np.uint16(0xCAFE)               # fp16 -13.98..: finite, never an integer
SENT32 = np.uint32(0xCAFEBABE)
SENT64 = np.int64(0x0123456789ABCDEF)
SPARE_ROWS = 3
ACT_NONE, ACT_GEGLU = 0, 4
BM, BK = 128, 64                         # the kernel's tile rows and K step


def pad8(n):
    return (n + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------------------------- cells
@dataclass
class Conv:
    B: int
    H: int
    W: int
    Cin: int
    Cout: int
    KH: int = 3
    KW: int = 3
    stride: int = 1
    pad_t: int = 1
    pad_l: int = 1
    ups: int = 1
    tstride: int = 1
    out_hw: tuple = None                 # None: the forward formula on the (upsampled) input
    fwd: tuple = None                    # dgrad cells: (stride, pad, extra bottom/right pad) of the forward conv whose input gradient this is

    def hw_out(self):
        if self.out_hw is not None:
            return self.out_hw
        Hu, Wu = self.H * self.ups, self.W * self.ups
        return ((Hu + 2 * self.pad_t - self.KH) // self.stride + 1, (Wu + 2 * self.pad_l - self.KW) // self.stride + 1)


@dataclass
class Cell:
    name: str
    M: int = 0
    N: int = 0
    K: int = 0
    lda: int = 0                         # 0: K (tight) / K + 8 (padded)
    ldb: int = 0
    ldc: int = 0                         # 0: N (tight) / N + 8 (padded)
    ldr: int = 0                         # 0: N (tight) / N + 16 (padded)
    r_off: int = 0                       # the residual pointer sits this many halfs behind a 16-byte boundary
    alpha: float = 1.0
    bias: bool = False
    bias_rows: int = 0                   # rows_per_bias_row (0: none)
    residual: bool = False
    act: int = ACT_NONE
    conv: Conv = None
    heads: tuple = None                  # batched dense: (B, heads, d, Tq, Tk) — head slices of [B, T, heads * d] buffers
    gn: tuple = None                     # (groups, rows per image)
    ln: bool = False
    amp: int = 2                         # operands drawn from {-amp .. amp}
    split: bool = False                  # the schedule the cell is meant to reach: split-K or one launch
    loader: str = "dense"                # dense | chunk (Cin % 64 != 0, tap per 16-byte chunk) | uniform (Cin % 64 == 0, tap per K step)
    plain_ldc: bool = False              # the form does not allow ldc > N (LayerNorm tail: ln_out mirrors C)


def _conv(name, B, H, W, Cin, Cout, split=False, **kw):
    cell_kw = {k: kw.pop(k) for k in list(kw) if k in ("bias", "bias_rows", "residual", "gn", "amp")}
    c = Conv(B, H, W, Cin, Cout, **kw)
    return Cell(name, conv=c, split=split, loader="uniform" if Cin % 64 == 0 else "chunk", **cell_kw)


DENSE = [
    Cell("dense-130x72x40", 130, 72, 40),
    Cell("dense-130x72x200", 130, 72, 200, lda=208, ldb=216, bias=True, residual=True, alpha=0.5),
    Cell("dense-257x136x320", 257, 136, 320, bias=True, residual=True),
    Cell("dense-2x1280x320", 2, 1280, 320, bias=True),
    Cell("dense-300x8x512", 300, 8, 512, residual=True, alpha=0.5),
    Cell("dense-33x75x72", 33, 75, 72, bias=True, residual=True),          # N % 8 != 0: a ragged last 8-column chunk (not in the issue's list)
]
DENSE_SPLIT = [
    Cell("split-128x64x1024", 128, 64, 1024, amp=1, split=True),
    Cell("split-77x328x1160", 77, 328, 1160, amp=1, split=True, bias=True, residual=True, alpha=0.5),      # 19 K steps, the last one 8 wide
    Cell("split-64x64x1216", 64, 64, 1216, amp=1, split=True),                                             # 19 K steps: no kps divides them
    Cell("split-ln-128x1280x1280", 128, 1280, 1280, amp=1, split=True, ln=True, bias=True, residual=True, plain_ldc=True),
    Cell("split-77x90x1280", 77, 90, 1280, amp=1, split=True, bias=True, residual=True),                   # N % 4 != 0: the element-wise tail
    Cell("split-77x92x1280", 77, 92, 1280, amp=1, split=True, bias=True, residual=True, ldr=96, r_off=2),  # N % 4 == 0, residual rows 4 bytes off
]
BATCHED = [
    Cell("heads-d24", heads=(2, 2, 24, 70, 45), alpha=0.5),
    Cell("heads-d72", heads=(2, 2, 72, 70, 45), alpha=0.5),
]
CONV_CHUNK = [
    _conv("conv-c8-9x7", 2, 9, 7, 8, 72, bias=True),
    _conv("conv-c40-s2-10x6", 2, 10, 6, 40, 72, stride=2, residual=True),
    _conv("conv-c72-ups-5x3", 2, 5, 3, 72, 40, ups=2, bias=True),
    _conv("conv-c136-dgrad-vae-down-12x8", 2, 6, 4, 136, 40, split=True, pad_t=2, pad_l=2, tstride=2, out_hw=(12, 8), fwd=(2, 0, 1)),
    _conv("conv-c48-dgrad-s2-10x6", 2, 5, 3, 48, 24, pad_t=1, pad_l=1, tstride=2, out_hw=(10, 6), fwd=(2, 1, 0)),
    _conv("conv-c24-1x1-9x7", 2, 9, 7, 24, 72, KH=1, KW=1, pad_t=0, pad_l=0, bias=True),
    _conv("conv-c16-pad-2-1-9x7", 2, 9, 7, 16, 24, pad_t=2, pad_l=1, out_hw=(11, 7)),                     # pad_t != pad_l (not in the issue's list)
]
CONV_UNIFORM = [
    _conv("conv-c64-9x7", 2, 9, 7, 64, 72, bias=True, residual=True),
    # K = 1152 is 18 K steps: at these sizes the plan splits them in two, so the Cin 128 cells reach their loader on the split-K schedule and
    # Cin 64 twins (9 K steps) reach it in one launch
    _conv("conv-c128-s2-10x6", 2, 10, 6, 128, 72, split=True, stride=2),
    _conv("conv-c128-vae-down-12x8", 2, 12, 8, 128, 72, split=True, stride=2, pad_t=0, pad_l=0, out_hw=(6, 4), bias=True),
    _conv("conv-c128-dgrad-vae-down-12x8", 2, 6, 4, 128, 72, split=True, pad_t=2, pad_l=2, tstride=2, out_hw=(12, 8), fwd=(2, 0, 1)),
    _conv("conv-c64-s2-10x6", 2, 10, 6, 64, 72, stride=2),
    _conv("conv-c64-vae-down-12x8", 2, 12, 8, 64, 72, stride=2, pad_t=0, pad_l=0, out_hw=(6, 4), bias=True),
    _conv("conv-c64-dgrad-vae-down-12x8", 2, 6, 4, 64, 72, pad_t=2, pad_l=2, tstride=2, out_hw=(12, 8), fwd=(2, 0, 1)),
    _conv("conv-c64-ups-5x3", 2, 5, 3, 64, 72, ups=2, bias=True),
    _conv("conv-c192-1x1-9x7", 2, 9, 7, 192, 72, KH=1, KW=1, pad_t=0, pad_l=0),
    _conv("conv-c64-b3-5x4-image-bias", 3, 5, 4, 64, 72, bias=True, bias_rows=20),                        # H_out W_out = 20: one tile holds all three images
    _conv("conv-c64-pad-2-1-9x7", 2, 9, 7, 64, 24, pad_t=2, pad_l=1, out_hw=(11, 7)),                     # pad_t != pad_l (not in the issue's list)
]
CONV_SPLIT = [
    _conv("conv-split-c128-8x8", 1, 8, 8, 128, 64, split=True, amp=1, bias=True),                          # 18 K steps: a split of 9 starts at channel 64 of tap 4
    _conv("conv-split-c320-b2-8x8", 2, 8, 8, 320, 64, split=True, amp=1, bias=True, bias_rows=64, residual=True),
]
GEGLU = [
    Cell("geglu-77x128x16", 77, 128, 16, act=ACT_GEGLU, bias=True),
    Cell("geglu-split-77x128x1280", 77, 128, 1280, act=ACT_GEGLU, bias=True, amp=1, split=True),
    # per-image bias in front of the pairing (not in the issue's list): the contract's epilogue order on both schedules
    Cell("geglu-image-bias-80x128x16", 80, 128, 16, act=ACT_GEGLU, bias=True, bias_rows=40),
    Cell("geglu-split-image-bias-80x128x1280", 80, 128, 1280, act=ACT_GEGLU, bias=True, bias_rows=40, amp=1, split=True),
]


def _gn_cells():
    out = []
    for tag, N, groups, rows in (("cg4", 128, 32, 64), ("cg5", 160, 32, 64), ("cg6", 192, 32, 64), ("cg10", 320, 32, 64), ("g6-cg8", 48, 6, 64),
                                 ("g6-cg5", 30, 6, 64), ("rows100-cg5", 160, 32, 100)):
        out.append(Cell(f"gn-{tag}", 3 * rows, N, 64, gn=(groups, rows), bias=True, residual=True))
        out.append(Cell(f"gn-split-{tag}", 3 * rows, N, 1280, gn=(groups, rows), bias=True, residual=True, amp=1, split=True))
    out.append(_conv("gn-conv-c64-b3-8x8-cg5", 3, 8, 8, 64, 160, gn=(32, 64), bias=True, bias_rows=64, amp=1))
    out.append(_conv("gn-conv-c24-b3-8x8-cg5", 3, 8, 8, 24, 160, gn=(32, 64), bias=True, amp=1))
    return out


GN = _gn_cells()
ALL_CELLS = DENSE + DENSE_SPLIT + BATCHED + CONV_CHUNK + CONV_UNIFORM + CONV_SPLIT + GEGLU + GN
BY_NAME = {c.name: c for c in ALL_CELLS}
assert len(BY_NAME) == len(ALL_CELLS)


# ---------------------------------------------------------------------------------------------------------------- the contract
def coord(num, tstride, ups, n_in):
    """header lines "num_h = oh*stride + kh - pad_t ..." -> (input coordinate, valid); num an int64 array"""
    num = np.asarray(num, np.int64)
    valid = num >= 0
    if tstride == 2:
        valid = valid & (num % 2 == 0)
        num = num // 2
    if ups == 2:
        num = num // 2
    valid = valid & (num < n_in)
    return np.where(valid, num, 0), valid


def im2col(x, c):
    """x [B, H_in, W_in, Cin] -> A [B * H_out * W_out, KH * KW * Cin], m = (image, oh, ow), k = (kh, kw, c); invalid taps read 0"""
    Ho, Wo = c.hw_out()
    ih, vh = coord(np.arange(Ho)[:, None] * c.stride + np.arange(c.KH)[None, :] - c.pad_t, c.tstride, c.ups, c.H)      # [Ho, KH]
    iw, vw = coord(np.arange(Wo)[:, None] * c.stride + np.arange(c.KW)[None, :] - c.pad_l, c.tstride, c.ups, c.W)      # [Wo, KW]
    g = x[:, ih[:, None, :, None], iw[None, :, None, :], :]                                                            # [B, Ho, Wo, KH, KW, Cin]
    g = g * (vh[:, None, :, None] & vw[None, :, None, :])[None, ..., None]
    return g.reshape(c.B * Ho * Wo, c.KH * c.KW * c.Cin)


def gelu(x):
    erf = np.frompyfunc(math.erf, 1, 1)
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + erf(x * math.sqrt(0.5)).astype(np.float64))


@dataclass
class Probe:
    cell: Cell
    padded: bool
    M: int
    N: int
    K: int
    lda: int
    ldb: int
    ldc: int
    ldr: int
    a_buf: np.ndarray                    # float16, flat; the A pointer is its start
    b_buf: np.ndarray
    r_buf: np.ndarray = None             # the residual pointer is r_buf[r_off:]
    r_off: int = 0
    bias: np.ndarray = None              # float32 [N]
    br_buf: np.ndarray = None            # float32, flat [images (+ spare)][ld_bias_rows]
    ld_bias_rows: int = 0
    batch: tuple = (1, 1)
    strides: tuple = (0, 0, 0, 0, 0, 0)  # sa_o, sa_i, sb_o, sb_i, sc_o, sc_i
    c_elems: int = 0                     # elements of the C / C32 allocation
    ln_gamma: np.ndarray = None
    ln_beta: np.ndarray = None
    expect: np.ndarray = None            # float64 [batch, M, width]
    expect_sums: np.ndarray = None       # int64 [images, groups, 2]
    logical: dict = field(default_factory=dict)

    @property
    def width(self):
        return self.N // 2 if self.cell.act == ACT_GEGLU else self.N

    def z_base(self, z, which):
        zo, zi = divmod(z, self.batch[1])
        so, si = self.strides[2 * which:2 * which + 2]
        return so * zo + si * zi

    def c_index(self):
        """flat indices of the outputs in the C allocation, [batch, M, width]"""
        Z = self.batch[0] * self.batch[1]
        base = np.array([self.z_base(z, 2) for z in range(Z)], np.int64)
        return base[:, None, None] + np.arange(self.M, dtype=np.int64)[None, :, None] * self.ldc + np.arange(self.width, dtype=np.int64)[None, None, :]

    def outputs(self):
        """-> (C float16 flat, C32 float32 flat, gn_sums int64 [1 + images + 1, groups, 2] or None), as the caller hands them over: sentinel
        everywhere, the statistics of the problem's own images zero"""
        C = np.full(self.c_elems, SENT16, np.uint16).view(np.float16)
        C32 = np.full(self.c_elems, SENT32, np.uint32).view(np.float32)
        gn = None
        if self.cell.gn:
            groups, rows = self.cell.gn
            gn = np.full((self.M // rows + 2, groups, 2), SENT64, np.int64)
            gn[1:-1] = 0
        return C, C32, gn


def operand_a(p, z):
    """A(z, m, k) of the contract, read from the probe's buffer -> float64 [M, K]"""
    base = p.z_base(z, 0)
    a = p.a_buf.astype(np.float64)
    if p.cell.conv is None:
        return a[base + np.arange(p.M)[:, None] * p.lda + np.arange(p.K)[None, :]]
    c = p.cell.conv
    return im2col(a[base:base + c.B * c.H * c.W * c.Cin].reshape(c.B, c.H, c.W, c.Cin), c)


def reference(p):
    """-> (y float64 [batch, M, width] before the rounding to half, sums int64 [images, groups, 2] of the half-rounded y or None)"""
    Z = p.batch[0] * p.batch[1]
    b = p.b_buf.astype(np.float64)
    ys = []
    for z in range(Z):
        A = operand_a(p, z)
        Bm = b[p.z_base(z, 1) + np.arange(p.N)[:, None] * p.ldb + np.arange(p.K)[None, :]]
        v = p.cell.alpha * (A @ Bm.T)
        if p.bias is not None:
            v = v + p.bias.astype(np.float64)[None, :]
        if p.br_buf is not None:
            v = v + p.br_buf.astype(np.float64)[(np.arange(p.M) // p.cell.bias_rows)[:, None] * p.ld_bias_rows + np.arange(p.N)[None, :]]
        if p.cell.act == ACT_GEGLU:
            v = v[:, 0::2] * gelu(v[:, 1::2])
        if p.r_buf is not None:
            v = v + p.r_buf.astype(np.float64)[p.r_off + p.z_base(z, 2) + np.arange(p.M)[:, None] * p.ldr + np.arange(p.N)[None, :]]
        ys.append(v)
    y = np.stack(ys)
    sums = None
    if p.cell.gn:
        groups, rows = p.cell.gn
        h = y[0].astype(np.float16).astype(np.float64).reshape(p.M // rows, rows, groups, p.N // groups)
        sums = np.stack([np.rint(h.sum((1, 3)) * 2.0 ** FRAC_BITS), np.rint((h * h).sum((1, 3)) * 2.0 ** FRAC_BITS)], -1).astype(np.int64)
    return y, sums


# ---------------------------------------------------------------------------------------------------------------- builders
def _rng(cell):
    return np.random.default_rng(zlib.crc32(cell.name.encode()))


def _ints(g, shape, amp):
    return g.integers(-amp, amp + 1, size=shape).astype(np.int64)


def _nonzero(a):
    """the slice, with its zeros replaced by ones, in place"""
    a[a == 0] = 1


def _lay(rows_alloc, ld, block, poison):
    """block [rows, cols] in a [rows_alloc, ld] float16 allocation, NaN (padded) or zero around it"""
    buf = np.full((rows_alloc, ld), np.nan if poison else 0.0, np.float16)
    buf[:block.shape[0], :block.shape[1]] = block
    return buf.reshape(-1)


def _assert_exact(p, y, sums):
    """the conditions (on the inputs and the reference alone) under which a correct kernel's result is exact and order-independent"""
    c = p.cell
    Z = p.batch[0] * p.batch[1]
    m, e = math.frexp(c.alpha)
    assert m == 0.5, "alpha is a power of two"
    bound = 0.0
    for z in range(Z):
        A = operand_a(p, z)
        Bm = p.b_buf.astype(np.float64)[p.z_base(z, 1) + np.arange(p.N)[:, None] * p.ldb + np.arange(p.K)[None, :]]
        for t in (A, Bm):
            assert np.isfinite(t).all() and (t == np.rint(t)).all() and np.abs(t).max() <= 2048, "operands are integers that fp16 holds"
        bound = max(bound, (np.abs(A) @ np.abs(Bm).T).max() * abs(c.alpha))
    assert bound < 2.0 ** 24, "every fp32 partial sum, split-K partials included, is exact in any order"
    extra = 0.0
    for t in (p.bias, None if p.br_buf is None else p.br_buf[np.isfinite(p.br_buf)], None if p.r_buf is None else p.r_buf[np.isfinite(p.r_buf)]):
        if t is not None:
            t = t.astype(np.float64)
            assert (t == np.rint(t)).all(), "bias, per-image bias and residual are integers"
            extra += np.abs(t).max()
    assert bound + extra < 2.0 ** 22, "the epilogue's fp32 additions of multiples of alpha are exact"
    assert np.isfinite(y).all() and np.abs(y).max() <= 2048 and (y == y.astype(np.float16).astype(np.float64)).all(), "the result is an fp16 number"
    if c.gn:
        assert (y == np.rint(y)).all() and np.abs(y).max() <= 256, "statistics: 64 squares of a thread's partial stay below 2^24"
        assert sums.shape == (p.M // c.gn[1], c.gn[0], 2)
    if c.act == ACT_GEGLU:
        assert (y == np.rint(y)).all()


def build(cell, padded):
    """the probe of a cell in its tight or padded (poison + sentinel) layout; the drawn values are the same in both"""
    g = _rng(cell)
    if cell.heads is not None:
        p = _build_heads(cell, padded, g)
    else:
        p = _build_plain(cell, padded, g)
    y, sums = reference(p)
    _assert_exact(p, y, sums)
    p.expect, p.expect_sums = y, sums
    return p


def _build_plain(cell, padded, g):
    c = cell.conv
    spare = SPARE_ROWS if padded else 0
    logical = {}
    if c is None:
        M, N, K = cell.M, cell.N, cell.K
        A = _ints(g, (M, K), cell.amp)
        _nonzero(A[M - 1]), _nonzero(A[:, K - 8:])                         # the last (ragged) row of M; the last (ragged) K chunk
        lda = cell.lda or (K + 8 if padded else K)
        a_buf = _lay(M + spare, lda, A, padded)
        logical["A"] = A
    else:
        Ho, Wo = c.hw_out()
        M, N, K = c.B * Ho * Wo, c.Cout, c.KH * c.KW * c.Cin
        x = _ints(g, (c.B, c.H, c.W, c.Cin), cell.amp)
        _nonzero(x[:, 0]), _nonzero(x[:, -1]), _nonzero(x[:, :, 0]), _nonzero(x[:, :, -1])      # border pixels
        assert (x[:, [0, -1]] != 0).all() and (x[:, :, [0, -1]] != 0).all()
        lda = 0
        guard = np.full(2 * c.W * c.Cin + 64 if padded else 0, np.nan, np.float16)             # two image rows and a K step of NaN behind the input
        a_buf = np.concatenate([x.astype(np.float16).reshape(-1), guard])
        logical["x"] = x
    Bm = _ints(g, (N, K), cell.amp)
    _nonzero(Bm[N - 1]), _nonzero(Bm[:, K - 8:])                           # the last (ragged) row of N; the last (ragged) K chunk
    if cell.act == ACT_GEGLU:
        # interleaved (value, gate) columns.  Gate rows select ONE of A's first eight columns, which hold 0 / 1, with weight 16: the gate
        # pre-activation is 0 or 16, gelu of it 0 or 16 in float32, the output 16 * value or 0.  gelu of a value column is no integer.
        assert c is None
        A[:, :8] = g.integers(0, 2, size=(M, 8))
        A[M - 1, :8] = 1
        a_buf = _lay(M + spare, lda, A, padded)
        Bm[1::2] = 0
        Bm[1::2][np.arange(N // 2), np.arange(N // 2) % 8] = 16
        Bm[0::2, :8] = 0                                                   # values: the rest of K
        if K == 16:
            _nonzero(Bm[0::2, 8:])
    logical["B"] = Bm
    ldb = cell.ldb or (K + 8 if padded else K)
    b_buf = _lay(N + spare, ldb, Bm, padded)
    width = N // 2 if cell.act == ACT_GEGLU else N
    ldc = cell.ldc or (width + 8 if padded and not cell.plain_ldc else width)
    p = Probe(cell, padded, M, N, K, lda, ldb, ldc, 0, a_buf, b_buf, c_elems=(M + spare) * ldc, logical=logical)
    if cell.bias:
        p.bias = _ints(g, (N,), 3).astype(np.float32)
        if cell.act == ACT_GEGLU:
            p.bias[1::2] = 0                                               # the gate stays 0 / 16
    if cell.bias_rows:
        n_img = -(-M // cell.bias_rows)
        p.ld_bias_rows = N + 4 if padded else N
        br = _ints(g, (n_img, N), 3) + 4 * (np.arange(n_img)[:, None] % 3 - 1)          # images differ by more than the draw
        if cell.act == ACT_GEGLU:
            br[:, 1::2] = 0                                                # the gate stays 0 / 16
        buf = np.full((n_img + spare, p.ld_bias_rows), np.nan if padded else 0.0, np.float32)
        buf[:n_img, :N] = br
        p.br_buf = buf.reshape(-1)
    if cell.residual:
        p.ldr = cell.ldr or (N + 16 if padded else N)
        p.r_off = cell.r_off
        R = _ints(g, (M, N), 3)
        p.r_buf = np.concatenate([np.full(p.r_off, np.nan if padded else 0.0, np.float16), _lay(M + spare, p.ldr, R, padded)])
    if cell.ln:
        p.ln_gamma = (1.0 + 0.25 * g.standard_normal(N)).astype(np.float32)
        p.ln_beta = (0.25 * g.standard_normal(N)).astype(np.float32)
    if c is None:
        Araw = logical["A"]
        assert (Araw[M - 1] != 0).all() and (Araw[:, K - 8:] != 0).any(1).all()
    assert (Bm[N - 1] != 0).any() and ((Bm[:, K - 8:] != 0).any(1).all() or cell.act == ACT_GEGLU)
    return p


def _build_heads(cell, padded, g):
    """attention-score shaped: A = q [B, Tq, heads * d], B = k [B, Tk, heads * d], C [B, heads, Tq, pad8(Tk)]; z = (image, head).  The pad
    columns Tk .. ldc - 1 and the spare rows behind the last head carry the sentinel."""
    Bt, heads, d, Tq, Tk = cell.heads
    Cw = heads * d
    q = _ints(g, (Bt, Tq, Cw), cell.amp)
    k = _ints(g, (Bt, Tk, Cw), cell.amp)
    _nonzero(q[:, Tq - 1]), _nonzero(k[:, Tk - 1]), _nonzero(q[..., -8:]), _nonzero(k[..., -8:])
    ldc = pad8(Tk)
    tail = SPARE_ROWS * ldc if padded else 0
    nan_tail = np.full(64 if padded else 0, np.nan, np.float16)
    return Probe(cell, padded, Tq, Tk, d, Cw, Cw, ldc, 0, np.concatenate([q.astype(np.float16).reshape(-1), nan_tail]),
                 np.concatenate([k.astype(np.float16).reshape(-1), nan_tail]), batch=(Bt, heads),
                 strides=(Tq * Cw, d, Tk * Cw, d, heads * Tq * ldc, Tq * ldc), c_elems=Bt * heads * Tq * ldc + tail, logical=dict(q=q, k=k))


# ---------------------------------------------------------------------------------------------------------------- checks
def check(p, C=None, C32=None, gn=None):
    """the outputs of a run on p.outputs() -> None, or (family, message) of the first check that fails"""
    idx = p.c_index()
    for name, out, sent in (("C", C, SENT16), ("C32", C32, SENT32)):
        if out is None:
            continue
        bits = out.view(sent.dtype)
        untouched = np.ones(bits.size, bool)
        untouched[idx.reshape(-1)] = False
        bad = np.flatnonzero(untouched & (bits != sent))
        if bad.size:
            return "sentinel", f"{p.cell.name}: {name}: {bad.size} elements outside [M, {p.width}] were written, the first at row {bad[0] // p.ldc} column {bad[0] % p.ldc}"
        got = out[idx].astype(np.float64)
        if np.isnan(got).any():
            z, m, n = (int(t[0]) for t in np.nonzero(np.isnan(got)))
            return "poison", f"{p.cell.name}: {name}: {int(np.isnan(got).sum())} outputs are NaN (a read outside the problem), the first at z {z} m {m} n {n}"
        if not np.array_equal(got, p.expect):
            z, m, n = (int(t[0]) for t in np.nonzero(got != p.expect))
            fam = "pairing" if p.cell.act == ACT_GEGLU else "field"
            return fam, f"{p.cell.name}: {name}: {int((got != p.expect).sum())} outputs differ, the first at z {z} m {m} n {n}: {got[z, m, n]} for {p.expect[z, m, n]}"
    if gn is not None:
        if not (np.array_equal(gn[0], np.full_like(gn[0], SENT64)) and np.array_equal(gn[-1], np.full_like(gn[-1], SENT64))):
            return "sentinel", f"{p.cell.name}: statistics of an image outside the problem were written"
        if not np.array_equal(gn[1:-1], p.expect_sums):
            i, grp, w = (int(t[0]) for t in np.nonzero(gn[1:-1] != p.expect_sums))
            return "stats", (f"{p.cell.name}: {int((gn[1:-1] != p.expect_sums).sum())} statistics differ, the first at image {i} group {grp} "
                             f"{'sum of squares' if w else 'sum'}: {gn[1 + i, grp, w]} for {p.expect_sums[i, grp, w]}")
    return None


# ---------------------------------------------------------------------------------------------------------------- structural model
DEFECTS = ("drop_last_ragged_k_chunk", "split_tap_state_channel_0", "kh_kw_swapped", "pad_l_for_pad_t", "odd_tstride_taps_kept",
           "ups_floor_before_sign_test", "image_bias_row_of_tile_start", "residual_pitch_ldc", "geglu_pair_shifted", "full_store_on_ragged_chunk",
           "third_group_folded_into_second", "stats_second_image_to_first", "split_partial_left_out")


def _gather(buf, idx, mask):
    """buf[idx] where mask, 0 elsewhere, as float64; an index the allocation does not cover reads NaN"""
    idx = np.asarray(idx, np.int64)
    inside = (idx >= 0) & (idx < buf.size)
    v = np.where(inside, buf[np.clip(idx, 0, buf.size - 1)].astype(np.float64), np.nan)
    return np.where(mask, v, 0.0)


def _model_coord(num, tstride, ups, n_in, defect):
    num = np.asarray(num, np.int64)
    if defect == "ups_floor_before_sign_test" and ups == 2:
        num = np.fix(num / 2).astype(np.int64)                             # C's truncating division: -1 / 2 == 0, a tap in the padding turns valid
        ups = 1
    valid = num >= 0
    if tstride == 2:
        if defect != "odd_tstride_taps_kept":
            valid = valid & (num % 2 == 0)
        num = num >> 1
    if ups == 2:
        num = num >> 1
    valid = valid & (num < n_in)
    return np.where(valid, num, 0), valid


def model(p, splits=1, bn=64, defect=None):
    """A kernel of csrc/sd_gemm.hip's design in numpy, on the probe's BUFFERS: 128 x bn output tiles, 64-wide K steps loaded in 8-element chunks
    (dense / tap per chunk / wave-uniform tap state initialised at the split's first K step), `splits` K ranges of ceil(n_ktiles / splits) steps
    with fp32 partials and a tail pass, an epilogue on 8-column chunks (16-byte stores where the chunk is whole), statistics in three buckets per
    chunk.  Arithmetic in float64 on exact values — the probes make the order irrelevant.  -> (C, C32, gn) like Probe.outputs()."""
    assert defect is None or defect in DEFECTS
    c = p.cell.conv
    C, C32, gn = p.outputs()
    if p.cell.act == ACT_GEGLU:
        C32 = None                                                         # (the contract has no float output for GEGLU)
    n_kt = -(-p.K // BK)
    kps = -(-n_kt // splits)
    splits = -(-n_kt // kps)
    Z = p.batch[0] * p.batch[1]
    uniform = c is not None and c.Cin % BK == 0
    pad_t = c.pad_l if c is not None and defect == "pad_l_for_pad_t" else (c.pad_t if c is not None else 0)

    def k_in(kc):
        if defect == "drop_last_ragged_k_chunk" and p.K % BK:
            return kc + 8 < p.K
        return kc < p.K

    def taps(rows, kh, kw):
        """pixel offsets (in elements) and validity of output rows `rows` at tap (kh, kw); kh, kw broadcast against rows[:, None]"""
        if defect == "kh_kw_swapped":
            kh, kw = kw, kh
        Ho, Wo = c.hw_out()
        img, rem = np.divmod(rows, Ho * Wo)
        oh, ow = np.divmod(rem, Wo)
        ih, vh = _model_coord(oh[:, None] * c.stride - pad_t + kh, c.tstride, c.ups, c.H, defect)
        iw, vw = _model_coord(ow[:, None] * c.stride - c.pad_l + kw, c.tstride, c.ups, c.W, defect)
        return ((img[:, None] * c.H + ih) * c.W + iw) * c.Cin, vh & vw

    def a_tile(z, rows, kt, state):
        kk = kt * BK + np.arange(BK)
        kc = kk - kk % 8
        rin = (rows < p.M)[:, None]
        r = np.where(rows < p.M, rows, 0)
        if c is None:
            return _gather(p.a_buf, p.z_base(z, 0) + r[:, None] * p.lda + kk[None, :], rin & k_in(kc)[None, :])
        if uniform:
            t_kh, t_kw, t_c0 = state
            off, ok = taps(r, np.int64(t_kh), np.int64(t_kw))
            out = _gather(p.a_buf, off + t_c0 + np.arange(BK)[None, :], rin & ok)
            t_c0 += BK
            if t_c0 >= c.Cin:
                t_c0 = 0
                t_kw += 1
                if t_kw == c.KW:
                    t_kw, t_kh = 0, t_kh + 1
            state[:] = [t_kh, t_kw, t_c0]
            return out
        tap = np.minimum(kc // c.Cin, c.KH * c.KW - 1)
        ch = kk - (kc // c.Cin) * c.Cin
        off, ok = taps(r, (tap // c.KW)[None, :], (tap % c.KW)[None, :])
        return _gather(p.a_buf, off + ch[None, :], rin & ok & k_in(kc)[None, :])

    def b_tile(z, cols, kt):
        kk = kt * BK + np.arange(BK)
        n = np.where(cols < p.N, cols, 0)
        return _gather(p.b_buf, p.z_base(z, 1) + n[:, None] * p.ldb + kk[None, :], (cols < p.N)[:, None] & k_in(kk - kk % 8)[None, :])

    def epilogue(z, v, rows, cols, m0):
        """v [rows, cols] fp32 sums -> C / C32 / gn; m0: the tile's first row (None in the split-K tail, which has no tiles)"""
        rin, cin = rows < p.M, cols < p.N
        inside = rin[:, None] & cin[None, :]
        r, n = np.where(rin, rows, 0), np.where(cin, cols, 0)
        v = v * p.cell.alpha
        if p.bias is not None:
            v = v + np.where(cin, p.bias.astype(np.float64)[n], 0.0)[None, :]
        if p.br_buf is not None:
            br = r // p.cell.bias_rows
            if defect == "image_bias_row_of_tile_start" and m0 is not None:
                br = np.full_like(r, m0 // p.cell.bias_rows)
            v = v + _gather(p.br_buf, br[:, None] * p.ld_bias_rows + n[None, :], inside)
        cbase = p.z_base(z, 2)
        if p.cell.act == ACT_GEGLU:
            val, gate = v[:, 0::2], v[:, 1::2]
            if defect == "geglu_pair_shifted":
                val, gate = v[:, 1::2], np.concatenate([v[:, 2::2], np.zeros((v.shape[0], 1))], 1)
            o = (val.astype(np.float32) * gelu(gate).astype(np.float32)).astype(np.float16)
            keep = inside[:, 1::2]
            C[(cbase + r[:, None] * p.ldc + n[None, 0::2] // 2)[keep]] = o[keep]
            return
        if p.r_buf is not None:
            ldr = p.ldc if defect == "residual_pitch_ldc" else p.ldr
            v = v + _gather(p.r_buf, p.r_off + cbase + r[:, None] * ldr + n[None, :], inside)
        store = inside
        if defect == "full_store_on_ragged_chunk":
            store = rin[:, None] & ((cols - cols % 8) < p.N)[None, :]
        dst = cbase + r[:, None] * p.ldc + cols[None, :]
        store = store & (dst < p.c_elems)
        with np.errstate(over="ignore", invalid="ignore"):
            C[dst[store]] = v.astype(np.float16)[store]
            C32[dst[store]] = v.astype(np.float32)[store]
        if gn is not None:
            groups, grows = p.cell.gn
            cg = p.N // groups
            nc = cols - cols % 8
            g_lo = nc // cg
            split_c = (g_lo + 1) * cg - nc
            e = cols - nc
            bucket = (e >= split_c).astype(np.int64) + (e >= split_c + cg)
            if defect == "third_group_folded_into_second" and m0 is not None:
                bucket = np.minimum(bucket, 1)
            grp = np.where(cin, g_lo + bucket, 0)
            img = r // grows
            if defect == "stats_second_image_to_first" and m0 is not None:
                img = np.full_like(r, m0 // grows)
            h = np.nan_to_num(v.astype(np.float16).astype(np.float64))
            for w, t in enumerate((h, h * h)):
                np.add.at(gn[1:-1, :, w], (np.broadcast_to(img[:, None], t.shape)[inside], np.broadcast_to(grp[None, :], t.shape)[inside]),
                          np.rint(t * 2.0 ** FRAC_BITS).astype(np.int64)[inside])

    with np.errstate(invalid="ignore"):
        for z in range(Z):
            partial = np.zeros((splits, p.M, p.N)) if splits > 1 else None
            for m0 in range(0, p.M, BM):
                rows = m0 + np.arange(BM)
                for n0 in range(0, p.N, bn):
                    cols = n0 + np.arange(bn)
                    for s in range(splits):
                        kt0, kt1 = s * kps, min(s * kps + kps, n_kt)
                        state = None
                        if uniform:
                            tap = kt0 * BK // c.Cin
                            t_c0 = 0 if defect == "split_tap_state_channel_0" else kt0 * BK - tap * c.Cin
                            state = [tap // c.KW, tap % c.KW, t_c0]
                        acc = np.zeros((BM, bn))
                        for kt in range(kt0, kt1):
                            acc += a_tile(z, rows, kt, state) @ b_tile(z, cols, kt).T
                        if splits == 1:
                            epilogue(z, acc, rows, cols, m0)
                        else:
                            mm, nn = min(BM, p.M - m0), min(bn, p.N - n0)
                            partial[s, m0:m0 + mm, n0:n0 + nn] = acc[:mm, :nn]
            if splits > 1:
                use = partial[:-1] if defect == "split_partial_left_out" else partial
                epilogue(z, use.sum(0), np.arange(p.M), np.arange(p.N), None)
    return C, C32, gn
