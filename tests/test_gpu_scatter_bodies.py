"""The level classes of the fp16 grid scatter (third form, k_bin3_*) that tests/test_gpu_scatter_cell_records.py does not reach, BYTE FOR BYTE.

k_bin3_emit holds one compiled body per level class and a workgroup takes the one of its level.  The byte-for-byte file runs the 16-level
and the 4-level benchmark-shaped tables: the hashed narrow body and the dense body with the second counter class.  The tables here reach
the rest:

  dense_narrow   a dense level of 65 ... 128 bins (no second counter class) beside a hashed narrow level
  hashed_wide    hashed levels of 256 bins (512 counters, reservations by 512 threads, copy-out bin by bin) beside a two-counter dense level
  dense_wide     a dense level of more than 128 bins beside a hashed level of 512 bins
  tiled_narrow   gridtype 'tiled' on a level that wraps: the strided sum masked into a power-of-two table (GE_MODE_TILED2), 128 bins
  tiled_wide     the same with 256 bins

each with align_corners off and on and with linear and smoothstep interpolation.  The intended geometry is asserted from the encoder's own
offsets and the level formula, so that a change of defaults cannot turn a case into another class without failing here.

The sums are exact 64-bit fixed point, so the gradient table is a function of the multiset of addends: the restatement of the
byte-for-byte file (imported, not edited) gives the expected bytes for the hash tables; its hashed-level index rule is restated here
for the tiled tables (restate_tiled), and the two restatements are compared with each other on a hash table's dense level.

Shapes: the binned scatter serves launches of at least 2^20 (sample, level) pairs, so B is 2^20 / levels + 5000 rounded up (never a
multiple of the 2048-sample point block: the last block is ragged)."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_scatter_cell_records import (B3_K, B3_PTS, CHUNK, P1, P2, TABLES as CELL_TABLES, b3_fix, check_bytes, f32, half_rn, level_geometry,
                                           make_case, quantise, restate)

pytestmark = pytest.mark.gpu

TABLES = {
    "dense_narrow": dict(input_dim=3, num_levels=2, level_dim=2, base_resolution=72, log2_hashmap_size=19, desired_resolution=2048, gridtype='hash'),
    "hashed_wide": dict(input_dim=3, num_levels=3, level_dim=2, base_resolution=16, log2_hashmap_size=20, desired_resolution=2048, gridtype='hash'),
    "dense_wide": dict(input_dim=3, num_levels=2, level_dim=2, base_resolution=100, log2_hashmap_size=21, desired_resolution=2048, gridtype='hash'),
    "tiled_narrow": dict(input_dim=3, num_levels=2, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048, gridtype='tiled'),
    "tiled_wide": dict(input_dim=3, num_levels=2, level_dim=2, base_resolution=16, log2_hashmap_size=20, desired_resolution=2048, gridtype='tiled'),
}
# per table: (dense?, lowest and highest admitted bin count) of every level, align_corners off | on
CLASSES = {
    "dense_narrow": [(True, 65, 128), (False, 128, 128)],
    "hashed_wide": [(True, 1, 64), (False, 256, 256), (False, 256, 256)],
    "dense_wide": [(True, 129, 512), (False, 512, 512)],
    "tiled_narrow": [(True, 1, 64), (False, 128, 128)],
    "tiled_wide": [(True, 1, 64), (False, 256, 256)],
}


def batch(table):
    L = TABLES[table]["num_levels"]
    B = (1 << 20) // L + 1 + 5000
    assert B * L >= 1 << 20 and B % B3_PTS != 0
    return B


def encoder(table, align_corners=False, smooth=False):
    from customnerf_amd.gridencoder import GridEncoder
    cfg = TABLES[table] if table in TABLES else CELL_TABLES[table]
    return GridEncoder(**cfg, align_corners=align_corners, interpolation='smoothstep' if smooth else 'linear')


def assert_classes(enc, table):
    """the level classes the case is meant to run, from the encoder's own offsets and the level formula"""
    geo = level_geometry(enc)
    assert len(geo) == len(CLASSES[table])
    for (off, size, scale, res, step, dense), (want_dense, lo, hi) in zip(geo, CLASSES[table]):
        bins = (size + CHUNK - 1) // CHUNK
        assert dense == want_dense and lo <= bins <= hi, (table, size, step, dense, bins)
        if not dense:
            assert size == bins * CHUNK and (size & (size - 1)) == 0


def tiled_index(px, py, pz, step, size):
    """ge_index_m<GE_MODE_TILED2>: the strided sum over the dimensions whose stride still fits the table, masked (32-bit arithmetic)"""
    stride, index = 1, np.zeros_like(px)
    for p in (px, py, pz):
        if stride <= size:
            index = (index + p * np.uint64(stride)) & np.uint64(0xFFFFFFFF)
            stride = (stride * step) & 0xFFFFFFFF
    return index & np.uint64(size - 1)


def restate_tiled(enc, x, g_lbc):
    """restate() of the byte-for-byte file with the tiled index rule on the levels that wrap (everything else in its words: the float32
    operations of b3_pairs, the half rounding of the emit, the w0s / w1s / b3_fix sequence of the accumulate) -> gradient table"""
    geo = level_geometry(enc)
    acc = np.zeros((int(enc._offsets_host[-1]), 2), dtype=np.int64)
    inside = ~((x < 0) | (x > 1)).any(axis=1)
    for l, (off, size, scale, res, step, dense) in enumerate(geo):
        g = g_lbc[l].astype(np.float32)
        ok = inside & ((g[:, 0] != 0) | (g[:, 1] != 0))
        xs, gs = x[ok], g[ok]
        pos = (xs.astype(np.float64) * np.float64(scale) + (0.0 if enc.align_corners else 0.5)).astype(np.float32)
        pg = np.floor(pos)
        fr = pos - pg
        pg = pg.astype(np.uint64)
        if enc.interp_id == 1:
            fr = fr * fr * (f32(3.0) - f32(2.0) * fr)
        fx, fy, fz = fr[:, 0], fr[:, 1], fr[:, 2]
        oy, oz = f32(1) - fy, f32(1) - fz
        wyz = [oy * oz, fy * oz, oy * fz, fy * fz]
        fxq = np.minimum((fx * f32(65536.0)).astype(np.uint32), 65535).astype(np.float32)
        w1 = fxq * f32(1.0 / 65536.0)
        w0 = f32(1) - w1
        w1s, w0s = w1 * f32(16777216.0), w0 * f32(16777216.0)
        for q in range(4):
            y, z = pg[:, 1] + np.uint64(q & 1), pg[:, 2] + np.uint64(q >> 1)
            if dense:
                i0 = pg[:, 0] + y * np.uint64(step) + z * np.uint64(step * step)
                i1 = i0 + np.uint64(1)
                if enc.align_corners:
                    i0 = np.where(i0 >= size, i0 - np.uint64(size), i0)
                    i1 = np.where(i1 >= size, i1 - np.uint64(size), i1)
                m = i0 ^ i1
                paired = (m != 0) & ((m >> np.uint64(12)) == 0) & ((m & (m + np.uint64(1))) == 0)
            else:
                i0 = tiled_index(pg[:, 0], y, z, step, size)
                i1 = tiled_index(pg[:, 0] + np.uint64(1), y, z, step, size)
                m = i0 ^ i1
                paired = (m != 0) & (m < (1 << B3_K)) & ((m & (m + np.uint64(1))) == 0)
            assert i0.max(initial=0) < size and i1.max(initial=0) < size
            for ch in range(2):
                f = half_rn(wyz[q] * gs[:, ch])
                a0p, a1p = b3_fix(w0s * f), b3_fix(w1s * f)
                u0, u1 = (f32(1) - fx) * wyz[q], fx * wyz[q]
                a0s = b3_fix(half_rn(u0 * gs[:, ch]) * f32(16777216.0))
                a1s = b3_fix(half_rn(u1 * gs[:, ch]) * f32(16777216.0))
                np.add.at(acc[:, ch], off + i0.astype(np.int64), np.where(paired, a0p, a0s))
                np.add.at(acc[:, ch], off + i1.astype(np.int64), np.where(paired, a1p, a1s))
    return (acc.astype(np.float64) * (1.0 / 16777216.0)).astype(np.float32)


def expected(enc, x, g):
    if enc.gridtype == 'tiled':
        return restate_tiled(enc, x, g)
    want, poisoned, _ = restate(enc, x, g)
    assert not poisoned
    return want


def workspace(enc, B):
    from customnerf_amd._lib import lib, check
    L, C = enc.num_levels, enc.level_dim
    need = ctypes.c_uint64(0)
    check(lib.cnerf_grid_encode_backward_workspace_bytes(enc._offsets_host.ctypes.data, B, 3, C, L, L, float(np.log2(enc.per_level_scale)), enc.base_resolution, 1,
                                                         ctypes.addressof(need)))
    assert need.value > 0, "the launch must take the binned scatter, not the atomic kernel"
    return torch.empty(int(need.value) + 256, dtype=torch.uint8, device='cuda')


def scatter_into(enc, x, g_lbc, ws, out):
    """cnerf_grid_encode_backward into `out` through the caller's workspace (no synchronisation: launches queue back to back)"""
    from customnerf_amd._lib import lib, ptr, stream, check
    B, L, C = x.shape[0], enc.num_levels, enc.level_dim
    check(lib.cnerf_grid_encode_backward(ptr(g_lbc), ptr(x), enc._offsets_host.ctypes.data, ptr(out), B, 3, C, L, L, float(np.log2(enc.per_level_scale)),
                                         enc.base_resolution, None, None, enc.gridtype_id, int(enc.align_corners), enc.interp_id, 1, ptr(ws), ws.numel(), stream()))


def scatter(enc, x, g, ws=None):
    ws = workspace(enc, x.shape[0]) if ws is None else ws
    out = torch.zeros(int(enc._offsets_host[-1]), enc.level_dim, device='cuda')
    scatter_into(enc, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), ws, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("smooth", [False, True], ids=["linear", "smoothstep"])
@pytest.mark.parametrize("align_corners", [False, True], ids=["centres", "align"])
@pytest.mark.parametrize("table", list(TABLES))
def test_every_level_class_matches_the_restatement_byte_for_byte(table, align_corners, smooth):
    """make_case of the byte-for-byte file: uniform samples, a crowded cell, samples on both sides of every bin border of every dense
    level and in the border cell, two samples outside the unit cube, a third of the gradients exactly zero, a ragged last point block"""
    enc = encoder(table, align_corners, smooth)
    assert_classes(enc, table)
    x, g = make_case(enc, batch(table), seed=21)
    want = expected(enc, x, g)
    assert np.abs(want).max() > 1.0
    for lvl, (off, size, *_) in enumerate(level_geometry(enc)):
        assert np.abs(want[off:off + size]).max() > 0, f"level {lvl} must receive gradient"
    got = scatter(enc, x, g)
    check_bytes(got, want)
    assert np.array_equal(scatter(enc, x, g).view(np.uint32), got.view(np.uint32))         # a second launch in the same process: the same bits


def test_the_tiled_restatement_is_the_imported_one_on_dense_levels():
    """restate_tiled differs from the imported restatement in the index rule of the wrapped levels alone: on a table whose hashed level gets no
    gradient the two give the same bytes (no GPU work: the restatements against each other)"""
    enc = encoder("dense_narrow")
    x, g = make_case(enc, 70001, seed=22)
    g[1] = 0
    want, _, _ = restate(enc, x, g)
    assert np.array_equal(restate_tiled(enc, x, g).view(np.uint32), want.view(np.uint32)) and np.abs(want).max() > 0


def test_the_tiled_index_rule_is_the_forward_pass_index():
    """the wrapped tiled level's entries as the forward gather finds them: a table that holds its own entry index returns, at a grid point
    (all weight on one corner), the index restated here"""
    enc = encoder("tiled_narrow").cuda()
    off, size, scale, res, step, dense = level_geometry(enc)[1]
    assert not dense
    rng = np.random.default_rng(23)
    cell = rng.integers(0, res - 1, size=(4096, 3))
    x = quantise((cell + 0.5) / float(scale))                                             # pos = x * scale + 0.5 = cell + 1: the corner (cell + 1), weight one
    pos = (x.astype(np.float64) * np.float64(scale) + 0.5).astype(np.float32)
    keep = (pos == np.floor(pos)).all(axis=1) & (x <= 1).all(axis=1)
    x, pg = x[keep], np.floor(pos[keep]).astype(np.uint64)
    assert keep.sum() > 1000
    idx = tiled_index(pg[:, 0], pg[:, 1], pg[:, 2], step, size).astype(np.int64)
    with torch.no_grad():
        enc.embeddings.zero_()
        ent = torch.arange(size, device='cuda')
        enc.embeddings[off:off + size, 0] = (ent % 2048).float()                           # (exact in the half-precision table too)
        enc.embeddings[off:off + size, 1] = (ent // 2048).float()
        y = enc(torch.from_numpy(x).cuda() * 2 - 1, bound=1.0).float().cpu().numpy()
    assert np.array_equal(y[:, 2].astype(np.int64) + 2048 * y[:, 3].astype(np.int64), idx)


def hashed_capacity(enc, B):
    """b3_plan: record capacity of a hashed bin's region"""
    cap = 0
    for off, size, scale, res, step, dense in level_geometry(enc):
        if not dense:
            mean = B * 17 // 4 // ((size + CHUNK - 1) // CHUNK)
            cap = max(cap, mean + mean // 2 + 8192)
    return (cap + 1) & ~1


def crowd(enc, x, g, rows, seed):
    """`rows` samples inside ONE cell of the finest level, none with a zero gradient: their records land in at most eight entries of it"""
    off, size, scale, res, step, dense = level_geometry(enc)[-1]
    assert not dense
    rng = np.random.default_rng(seed)
    x[rows] = quantise((np.array([700.0, 901.0, 1203.0]) + 0.05 + 0.9 * rng.random((len(rows), 3))) / float(scale))
    g[:, rows] = (rng.standard_normal((enc.num_levels, len(rows), 2)) + 3.0).astype(np.float16)
    assert (g[:, rows] != 0).all()


@pytest.mark.parametrize("first", ["plain", "spill"])
def test_two_launches_back_to_back_on_one_workspace(first):
    """Two different batches through the SAME workspace, queued without a synchronisation in between: whatever the first launch leaves in the
    bin cursors, their spill flags, the run table and the service words must not reach the second.  `spill`: a third of the first batch sits
    in one cell of the finest (hashed) level, far more records than a bin's region holds, so those bins overflow, raise their spill flag and
    leave spilled runs behind; the second batch does not overflow."""
    enc = encoder("L16_T19")
    B = 65536 + 5000
    xa, ga = make_case(enc, B, seed=31)
    xb, gb = make_case(enc, B, seed=32)
    if first == "spill":
        rows = np.arange(30000, 54000)
        crowd(enc, xa, ga, rows, seed=33)
        assert len(rows) > hashed_capacity(enc, B), "the crowded cell's bins must overflow their regions"
    ws = workspace(enc, B)
    outs = [torch.zeros(int(enc._offsets_host[-1]), 2, device='cuda') for _ in range(2)]
    dev = [(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()) for x, g in ((xa, ga), (xb, gb))]
    for (xd, gd), out in zip(dev, outs):
        scatter_into(enc, xd, gd, ws, out)
    torch.cuda.synchronize()
    check_bytes(outs[0].cpu().numpy(), expected(enc, xa, ga))
    check_bytes(outs[1].cpu().numpy(), expected(enc, xb, gb))


@pytest.mark.parametrize("found_inf", [False, True], ids=["armed", "armed_found_inf"])
def test_the_armed_table_update_is_the_separate_adam_launch(found_inf):
    """cnerf_grid_backward_adam armed (and armed under a raised found_inf: no update, gradients cleared) on a table with a dense narrow and a
    hashed narrow level and on one with a two-counter dense level and wide hashed levels: parameters, moments, fp16 shadow and gradient table
    equal those of the un-armed scatter followed by cnerf_adam_step_scaled, bit for bit"""
    from customnerf_amd._lib import lib, ptr, stream, check, GridAdam
    for table in ("dense_narrow", "hashed_wide"):
        enc = encoder(table).cuda()
        B = batch(table)
        x, g = make_case(enc, B, seed=41)
        xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
        ws = workspace(enc, B)
        gen = torch.Generator(device='cuda').manual_seed(42)
        p0 = (torch.rand(enc.embeddings.shape, device='cuda', generator=gen) - 0.5) * 0.2
        m0 = torch.rand(enc.embeddings.shape, device='cuda', generator=gen) * 1e-3
        v0 = torch.rand(enc.embeddings.shape, device='cuda', generator=gen) * 1e-6
        state0 = torch.tensor([128.0, 3.0, 1.0 if found_inf else 0.0, 17.0], device='cuda')
        outs = []
        for fused in (False, True):
            p, m, v, st = p0.clone(), m0.clone(), v0.clone(), state0.clone()
            grad = torch.zeros_like(p)
            ph = torch.zeros(p.shape, dtype=torch.half, device='cuda')
            if fused:
                cfg = GridAdam()
                cfg.p, cfg.g, cfg.m, cfg.v, cfg.p_half, cfg.n = p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), ph.data_ptr(), p.numel()
                cfg.lr, cfg.beta1, cfg.beta2, cfg.eps = 1e-2, 0.9, 0.99, 1e-15
                cfg.scaler_state, cfg.extra_inv, cfg.zero_grad = st.data_ptr(), 1.0, 1
                check(lib.cnerf_grid_backward_adam(ctypes.addressof(cfg)))
            try:
                scatter_into(enc, xd, gd, ws, grad)
                done = ctypes.c_int(0)
                if fused:
                    check(lib.cnerf_grid_backward_adam_consumed(ctypes.addressof(done)))
            finally:
                check(lib.cnerf_grid_backward_adam(None))
            if fused:
                assert done.value == 1, "the armed step must ride on this backward pass"
            else:
                check(lib.cnerf_adam_step_scaled(ptr(p), ptr(grad), ptr(m), ptr(v), ptr(ph), p.numel(), 1e-2, 0.9, 0.99, 1e-15, ptr(st), 1.0, 1, stream()))
            torch.cuda.synchronize()
            outs.append((p, m, v, ph, grad))
        for name, a, b in zip(("p", "m", "v", "p_half", "g"), *outs):
            assert torch.equal(a, b), (table, name)
        assert float(outs[0][4].abs().max()) == 0.0                                         # zero_grad: cleared either way
        assert torch.equal(outs[0][0], p0) == found_inf                                     # a skipped step leaves the parameters alone
