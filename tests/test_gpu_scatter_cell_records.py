"""The fp16 grid scatter (third form, k_bin3_*) against a numpy restatement, BYTE FOR BYTE.

The sums of the third form are exact 64-bit fixed point, so the gradient table is a function of the multiset of addends alone.  The
restatement forms every addend as the kernels do — the float32 operations of b3_pairs, the half rounding of the emit's phase 2, the
w0s / w1s / b3_fix sequence of b3_push_record — sums in int64 and converts as bn_acc_to_float does.  It describes the scatter before and
after the emit learnt to take ONE LDS ticket for the four pair records of a sample whose eight corners share a bin (its second counter
class on the coarse dense levels): that change moves records inside a run and nothing else, so the same bytes must come out.  The cases aim at what the one-ticket path can get
wrong: cells that straddle a bin border (they keep a ticket per record) on either side of cells that do not, the border cell itself,
(the five dense levels of the 16-level table have 17 / 24 / 32 / 44 / 60 lines per axis with align_corners off, one fewer with it on: a cell
spans S^2 + S + 1 entries, so 7.5 / 15 / 26 / 48 / 89 % of the cells straddle one of the 4096-entry bins)
align_corners wrap-around, a crowded cell, a ragged last point block, zero and non-finite gradients, a point block that overflows the
emit's staging area with both kinds of sample in it.

Shapes: the binned scatter serves launches of at least 2^20 (sample, level) pairs — below that the entry point takes the atomic kernel —
so B is 65536 + 5000 on the 16-level table and 262144 + 5000 on the 4-level one (neither a multiple of the 2048-sample point block).
Which form of the binned scatter ran, how many records a block staged and whether it spilled cannot be read back from Python; the tests
assert what shows the path from outside: the workspace query (non-zero only when the launch is binned) and, for the spill, the record
count of the block as the restatement counts it against the staging capacity restated here."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 4096            # BN_CHUNK: entries per bin
B3_K = 7                # interleaved bins of the hashed levels: an x-pair is one record while x ^ (x + 1) < 2^7
B3_PTS = 2048           # samples per point block
B3_CAP = B3_PTS * 4 + 640
P1, P2 = 2654435761, 805459861
_libm = ctypes.CDLL("libm.so.6")
_libm.exp2f.restype = ctypes.c_float
_libm.exp2f.argtypes = [ctypes.c_float]
f32 = np.float32

TABLES = {
    "L16_T19": dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048, gridtype='hash'),
    "L4_T14": dict(input_dim=3, num_levels=4, level_dim=2, base_resolution=16, log2_hashmap_size=14, desired_resolution=2048, gridtype='hash'),
}
BATCH = {"L16_T19": 65536 + 5000, "L4_T14": 262144 + 5000}


def encoder(table, align_corners, smooth):
    from customnerf_amd.gridencoder import GridEncoder
    return GridEncoder(**TABLES[table], align_corners=align_corners, interpolation='smoothstep' if smooth else 'linear')


def level_geometry(enc):
    """ge_levels (grid_common.h): per level (offset, size, scale, resolution, step, dense?)"""
    off = enc._offsets_host
    S = f32(float(np.log2(enc.per_level_scale)))
    out = []
    for l in range(enc.num_levels):
        size = int(off[l + 1] - off[l])
        scale = f32(f32(_libm.exp2f(f32(f32(l) * S))) * f32(enc.base_resolution)) - f32(1.0)
        res = int(np.ceil(scale)) + 1
        step = res if enc.align_corners else res + 1
        dense = step ** 3 <= size
        assert dense or (size & (size - 1)) == 0, "hashed levels of the test tables are powers of two (GE_MODE_HASH2)"
        out.append((int(off[l]), size, f32(scale), res, step, dense))
    return out


def b3_fix(a):
    """b3_fix: llrint(a) as a 64-bit pattern by the 1.5 * 2^52 trick (an infinity gives the same arbitrary finite pattern as on the device)"""
    with np.errstate(over='ignore'):
        y = a.astype(np.float64) + 6755399441055744.0
        return (y.view(np.uint64) - np.uint64(0x4338000000000000)).view(np.int64)


def half_rn(a):
    with np.errstate(over='ignore'):
        return a.astype(np.float16).astype(np.float32)


def restate(enc, x, g_lbc):
    """-> (gradient table float32 [entries, 2] for a zeroed destination, poisoned flat entries, records per (level, point block))"""
    geo = level_geometry(enc)
    B = x.shape[0]
    acc = np.zeros((int(enc._offsets_host[-1]), 2), dtype=np.int64)
    poisoned = []
    n_blocks = (B + B3_PTS - 1) // B3_PTS
    records = np.zeros((enc.num_levels, n_blocks), dtype=np.int64)
    inside = ~((x < 0) | (x > 1)).any(axis=1)
    for l, (off, size, scale, res, step, dense) in enumerate(geo):
        g = g_lbc[l].astype(np.float32)                                            # [B, 2], the fp16 gradient as loaded
        with np.errstate(invalid='ignore'):
            ok = inside & ((g[:, 0] != 0) | (g[:, 1] != 0))
        xs, gs, rows = x[ok], g[ok], np.nonzero(ok)[0]
        # pos = fma(in, scale, 0.5 | 0): the product and the sum are exact in float64 for coordinates that are multiples of 2^-24 (asserted by the callers)
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
        bad = ~(np.abs(gs) <= 65504.0).all(axis=1)
        n_rec = np.zeros(len(rows), dtype=np.int64)
        for q in range(4):
            y, z = pg[:, 1] + (q & 1), pg[:, 2] + (q >> 1)
            if dense:
                i0 = pg[:, 0] + y * step + z * step * step
                i1 = i0 + 1
                if enc.align_corners:
                    i0 = np.where(i0 >= size, i0 - size, i0)
                    i1 = np.where(i1 >= size, i1 - size, i1)
                m = i0 ^ i1
                paired = (m != 0) & ((m >> 12) == 0) & ((m & (m + 1)) == 0)
            else:
                h = ((y * P1) & 0xFFFFFFFF) ^ ((z * P2) & 0xFFFFFFFF)
                i0 = (pg[:, 0] ^ h) & (size - 1)
                i1 = ((pg[:, 0] + 1) ^ h) & (size - 1)
                m = i0 ^ i1
                paired = (m != 0) & (m < (1 << B3_K)) & ((m & (m + 1)) == 0)
            assert i0.max(initial=0) < size and i1.max(initial=0) < size
            if q == 0:
                poisoned += list(off + i0[bad].astype(np.int64))
            n_rec += np.where(paired, 1, 2)
            for ch in range(2):
                with np.errstate(over='ignore', invalid='ignore'):
                    f = half_rn(wyz[q] * gs[:, ch])                                # the pair record's value
                    a0p, a1p = b3_fix(w0s * f), b3_fix(w1s * f)
                    u0, u1 = (f32(1) - fx) * wyz[q], fx * wyz[q]                   # singles: the corner's own weight, rounded to half with the gradient
                    a0s = b3_fix(half_rn(u0 * gs[:, ch]) * f32(16777216.0))
                    a1s = b3_fix(half_rn(u1 * gs[:, ch]) * f32(16777216.0))
                np.add.at(acc[:, ch], off + i0.astype(np.int64), np.where(paired, a0p, a0s))
                np.add.at(acc[:, ch], off + i1.astype(np.int64), np.where(paired, a1p, a1s))
        np.add.at(records[l], rows // B3_PTS, n_rec)
    return (acc.astype(np.float64) * (1.0 / 16777216.0)).astype(np.float32), sorted(set(int(p) for p in poisoned)), records


def scatter(enc, x, g_lbc, watch=None):
    """cnerf_grid_encode_backward with its workspace, into a zeroed table -> float32 [entries, 2] on the host.  watch: a loss scaler's
    {scale, growth_tracker, found_inf, good_steps} on the device, watched (cnerf_scaler_watch) for the duration of the launch."""
    from customnerf_amd._lib import lib, ptr, stream, check
    B, L, C = x.shape[0], enc.num_levels, enc.level_dim
    S = float(np.log2(enc.per_level_scale))
    need = ctypes.c_uint64(0)
    check(lib.cnerf_grid_encode_backward_workspace_bytes(enc._offsets_host.ctypes.data, B, 3, C, L, L, S, enc.base_resolution, 1, ctypes.addressof(need)))
    assert need.value > 0, "the launch must take the binned scatter, not the atomic kernel"
    ws = torch.empty(int(need.value) + 256, dtype=torch.uint8, device='cuda')
    xd = torch.from_numpy(x).cuda()
    gd = torch.from_numpy(g_lbc).cuda()
    out = torch.zeros(int(enc._offsets_host[-1]), C, device='cuda')
    if watch is not None:
        check(lib.cnerf_scaler_watch(ptr(watch)))
    try:
        check(lib.cnerf_grid_encode_backward(ptr(gd), ptr(xd), enc._offsets_host.ctypes.data, ptr(out), B, 3, C, L, L, S, enc.base_resolution,
                                             None, None, enc.gridtype_id, int(enc.align_corners), enc.interp_id, 1, ptr(ws), ws.numel(), stream()))
        torch.cuda.synchronize()
    finally:
        if watch is not None:
            check(lib.cnerf_scaler_watch(None))
    return out.cpu().numpy()


def block_layout(enc, x, g_lbc, lvl, block):
    """The run layout of one point block on a dense level of at most 64 bins (align_corners off), as b3_emit<true> (k_bin3_emit) builds it: per bin c,
    n_one[c] samples whose lowest and highest corner share bin c (one ticket, 4 n_one[c] slots, pair-major) in front of n_tick[c] ticketed
    records; the runs in bin order.  -> (n_one [bins], n_tick [bins], first slot of each bin's run)"""
    assert not enc.align_corners
    off, size, scale, res, step, dense = level_geometry(enc)[lvl]
    nch = (size + CHUNK - 1) // CHUNK
    assert dense and nch <= 64
    rows = np.arange(block * B3_PTS, min((block + 1) * B3_PTS, x.shape[0]))
    xs, g = x[rows], g_lbc[lvl][rows].astype(np.float32)
    ok = ~((xs < 0) | (xs > 1)).any(axis=1) & ((g[:, 0] != 0) | (g[:, 1] != 0))
    pos = (xs[ok].astype(np.float64) * np.float64(scale) + 0.5).astype(np.float32)
    pg = np.floor(pos).astype(np.int64)
    lin = pg[:, 0] + pg[:, 1] * step + pg[:, 2] * step * step
    one = (lin // CHUNK) == ((lin + step * step + step + 1) // CHUNK)
    n_one = np.bincount(lin[one] // CHUNK, minlength=nch)
    n_tick = np.zeros(nch, dtype=np.int64)
    for q in range(4):
        i0 = lin[~one] + (q & 1) * step + (q >> 1) * step * step
        single = (i0 // CHUNK) != ((i0 + 1) // CHUNK)                              # the x-pair crosses a bin border: two single records
        n_tick += np.bincount(i0 // CHUNK, minlength=nch) + np.bincount((i0 + 1)[single] // CHUNK, minlength=nch)
    start = np.concatenate([[0], np.cumsum(4 * n_one + n_tick)[:-1]])
    return n_one, n_tick, start


def quantise(x):
    """coordinates as multiples of 2^-24 in [0, 1] (what rng.random(float32) gives): the restatement's float64 fma is then exact"""
    return (np.round(np.asarray(x, dtype=np.float64) * 2.0 ** 24) / 2.0 ** 24).astype(np.float32)


def cell_point(geo_l, align_corners, lin, frac):
    """a point inside the cell whose lowest corner is entry `lin` of a dense level, at fraction `frac` of the cell along every axis"""
    off, size, scale, res, step, dense = geo_l
    gx, gy, gz = lin % step, (lin // step) % step, lin // (step * step)
    shift = 0.0 if align_corners else 0.5
    return [(c + frac - shift) / float(scale) for c in (gx, gy, gz)]


def make_case(enc, B, seed):
    """uniform samples + a crowded level-0 cell + the bin borders of every dense level + exact 0 / 1 coordinates; a third of the gradients zero"""
    rng = np.random.default_rng(seed)
    geo = level_geometry(enc)
    x = rng.random((B, 3), dtype=np.float32)
    x[0], x[1], x[2], x[3] = 0.0, 1.0, (0.0, 1.0, 0.0), (1.0, 0.0, 1.0)
    x[4, 0], x[5, 2] = -0.01, 1.001                                                # out of range: no records
    # every sample of 3000 in ONE cell of level 0 (crowding, register combining, many records of one key in a run); they straddle the
    # point-block border at 4096
    x[3000:6000] = quantise(np.array(cell_point(geo[0], enc.align_corners, 5 + 7 * geo[0][4] + 3 * geo[0][4] ** 2, 0.0)) +
                            rng.random((3000, 3)) * 0.9 / float(geo[0][2]))
    # cells whose span [lin, lin + S^2 + S + 1] holds entry 4096 k (they straddle: a ticket per record), the border cell itself
    # (lin = 4096 k), the first cell past the span and the last one before it — on every dense level, every k
    row = 8000
    n_border = 0
    for gl in geo:
        off, size, scale, res, step, dense = gl
        if not dense:
            continue
        span = step * step + step + 1
        for k in range(1, (size + CHUNK - 1) // CHUNK):
            for lin in (CHUNK * k - span - 1, CHUNK * k - span, CHUNK * k - step, CHUNK * k - 1, CHUNK * k, CHUNK * k + 1):
                gx, gy, gz = lin % step, (lin // step) % step, lin // (step * step)
                if lin < 0 or max(gx, gy, gz) >= res - (1 if enc.align_corners else 0) or row + 3 > 60000:
                    continue                                                       # (no such cell inside the unit cube)
                placed = 0
                for frac in (0.25, 0.5, 0.8125):
                    pt = quantise(cell_point(gl, enc.align_corners, lin, frac))
                    if pt.min() < 0 or pt.max() > 1:
                        continue                                                   # (the half cells at the faces of the cube)
                    x[row] = pt
                    row += 1
                    placed += 1
                n_border += placed > 0
    assert n_border >= 4 * sum(1 for gl in geo if gl[5] and gl[1] > CHUNK)          # (the 4-level table with align_corners has no dense level beyond one bin)
    inside = ~((x < 0) | (x > 1)).any(axis=1)
    assert np.array_equal(x[inside], quantise(x[inside])) and (~inside).sum() == 2
    L = enc.num_levels
    g = rng.standard_normal((L, B, 2)).astype(np.float16)
    g[:, rng.random(B) < 1.0 / 3.0] = 0                                            # a third of the samples: exactly zero on every level
    g[:, 3000:6000][:, ::7] = 0
    return x, g


def check_bytes(got, want, poisoned=()):
    mask = np.ones(got.shape, dtype=bool)
    for p in poisoned:
        assert np.isnan(got[p, 0]), f"entry {p} must carry the non-finite gradient"
        mask[p, 0] = False
    assert not np.isnan(got[mask]).any()
    diff = np.nonzero((got.view(np.uint32) != want.view(np.uint32)) & mask)
    assert diff[0].size == 0, f"{diff[0].size} words differ, first at entry {diff[0][:5]}: {got[diff][:5]} vs {want[diff][:5]}"


@pytest.mark.parametrize("smooth", [False, True], ids=["linear", "smoothstep"])
@pytest.mark.parametrize("align_corners", [False, True], ids=["centres", "align"])
@pytest.mark.parametrize("table", list(TABLES))
def test_scatter_matches_the_restatement_byte_for_byte(table, align_corners, smooth):
    enc = encoder(table, align_corners, smooth)
    x, g = make_case(enc, BATCH[table], seed=7)
    want, poisoned, _ = restate(enc, x, g)
    assert not poisoned and np.abs(want).max() > 1.0
    got = scatter(enc, x, g)
    check_bytes(got, want)
    assert np.array_equal(scatter(enc, x, g).view(np.uint32), got.view(np.uint32))         # a second launch in the same process: the same bits


def test_non_finite_gradients_poison_their_entries_and_raise_found_inf():
    """A non-finite gradient on a one-ticket sample of a dense level, on a sample of the same level whose cell straddles a bin border (a ticket
    per record) and on a hashed level: each poisons the entry of its lowest corner and raises the watched scaler's found_inf
    (cnerf_scaler_watch); every other word is the restatement's, and a finite launch leaves found_inf at 0."""
    enc = encoder("L16_T19", False, False)
    geo = level_geometry(enc)
    x, g = make_case(enc, BATCH["L16_T19"], seed=9)
    state = torch.tensor([65536.0, 0.0, 0.0, 0.0], device='cuda')
    want, poisoned, _ = restate(enc, x, g)
    assert not poisoned
    check_bytes(scatter(enc, x, g, watch=state), want)
    assert state.cpu().tolist() == [65536.0, 0.0, 0.0, 0.0], "a finite launch must leave the scaler state alone"
    row, row_s = 20000, 20001
    x[row] = quantise([0.3171, 0.6113, 0.4219])                                    # generic fractions: no zero weight meets the infinity
    off, size, scale, res, step, dense = geo[2]
    span = step * step + step + 1
    lin_s = next(l for l in range(CHUNK - span + 1, CHUNK) if 1 <= min(l % step, (l // step) % step, l // (step * step)) and max(l % step, (l // step) % step, l // (step * step)) < res - 1)
    x[row_s] = quantise(cell_point(geo[2], False, lin_s, 0.3))                     # level 2: the cell's span holds entry 4096
    g[:, [row, row_s]] = 1.0
    g[2, row, 1] = np.inf                                                          # a dense level, one-ticket sample
    g[2, row_s, 0] = np.inf                                                        # the same level, a straddling sample
    g[9, row, 0] = -np.inf                                                         # a hashed level
    n_one, n_tick, _ = block_layout(enc, x, g, 2, row // B3_PTS)
    pos = (x[[row, row_s]].astype(np.float64) * np.float64(scale) + 0.5).astype(np.float32)
    lin = (np.floor(pos).astype(np.int64) * [1, step, step * step]).sum(axis=1)
    assert lin[0] // CHUNK == (lin[0] + span) // CHUNK and lin[1] == lin_s and lin[1] // CHUNK != (lin[1] + span) // CHUNK
    assert n_one.sum() > 0 and n_tick.sum() > 0
    want, poisoned, _ = restate(enc, x, g)
    assert len(poisoned) == 3
    for _ in range(2):
        state[2] = 0.0
        check_bytes(scatter(enc, x, g, watch=state), want, poisoned)
        assert state.cpu().tolist() == [65536.0, 0.0, 1.0, 0.0], "found_inf must be raised, and nothing else of the state touched"
    state[2] = 0.0
    g[2, row, 1] = g[9, row, 0] = 1.0                                              # the straddling sample alone: the per-record branch raises it too
    want, poisoned, _ = restate(enc, x, g)
    assert len(poisoned) == 1
    check_bytes(scatter(enc, x, g, watch=state), want, poisoned)
    assert state[2].item() == 1.0


def test_a_block_that_overflows_the_staging_area_with_both_kinds_of_sample():
    """Point block 3 of level 3 (a dense level of 44 lines per axis, 21 bins; a cell spans 1981 entries, so 48 % of the cells straddle a bin
    border): 1500 samples in the cell whose first x-pair crosses entry 4096 k - 1 | 4096 k — two single records and three pair records each, a
    ticket per record, in bins k - 1 and k — and 548 in a cell that lies wholly inside bin k + 1 and takes the one-ticket path, duplicates
    of a few points.  9692 records against a staging capacity of 8832: the runs go in bin order, so the one-ticket slots of bin k + 1 start at
    7500 and those from 8832 on go straight to the block's region (the spill rule) — asserted from the restated run layout, since no count
    can be read back from the device."""
    enc = encoder("L16_T19", False, False)
    geo = level_geometry(enc)
    B = BATCH["L16_T19"]
    x, g = make_case(enc, B, seed=11)
    lvl = 3
    off, size, scale, res, step, dense = geo[lvl]
    span = step * step + step + 1
    assert dense and step == 44 and (size + CHUNK - 1) // CHUNK == 21

    def in_cube(l):
        c = (l % step, (l // step) % step, l // (step * step))
        return 1 <= min(c) and max(c) < res - 1

    k = next(k for k in range(1, size // CHUNK - 1) if in_cube(CHUNK * k - 1))
    lin_b = next(l for l in range(CHUNK * (k + 1), CHUNK * (k + 2) - span) if in_cube(l))
    rng = np.random.default_rng(12)
    b0 = 3 * B3_PTS
    pts_a = quantise(np.array(cell_point(geo[lvl], False, CHUNK * k - 1, 0.0)) + rng.random((16, 3)) * 0.9 / float(scale))
    pts_b = quantise(np.array(cell_point(geo[lvl], False, lin_b, 0.0)) + rng.random((16, 3)) * 0.9 / float(scale))
    x[b0:b0 + 1500] = pts_a[rng.integers(0, 16, 1500)]
    x[b0 + 1500:b0 + B3_PTS] = pts_b[rng.integers(0, 16, B3_PTS - 1500)]
    g[:, b0:b0 + B3_PTS] = rng.standard_normal((enc.num_levels, B3_PTS, 2)).astype(np.float16) + np.float16(3.0)      # (no zero gradient in the block)
    want, poisoned, records = restate(enc, x, g)
    assert not poisoned
    assert records[lvl, 3] == 1500 * 5 + 548 * 4 > B3_CAP, "the block must emit more records than the staging area holds"
    n_one, n_tick, start = block_layout(enc, x, g, lvl, 3)
    assert n_one[k + 1] == 548 and n_one.sum() == 548 and n_tick[k - 1] == 1500 and n_tick[k] == 6000 and n_tick.sum() == 7500
    assert start[k + 1] == 7500 < B3_CAP < start[k + 1] + 4 * n_one[k + 1], "one-ticket slots (run start + q n + r) on both sides of the staging capacity"
    got = scatter(enc, x, g)
    check_bytes(got, want)
    assert np.array_equal(scatter(enc, x, g).view(np.uint32), got.view(np.uint32))
