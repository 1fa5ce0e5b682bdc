"""The sample-major gather's workgroup shape (1024 threads x 4 samples on a 4096-sample tile, a barrier per level) and its XCD-contiguous tile
assignment on tables whose levels exceed an L2: cnerf_grid_encode_forward_ordered with traversal 1 must write, byte for byte, what the
level-major kernel (traversal 0, pinned to oracle/gridencoder_ref.c by test_gpu_gridencoder.py) writes, and nothing else."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 1024 * 4                               # GE_FAST_THREADS x GE_FAST_SPT (csrc/gridencoder.hip, which points back here): change them together
SIZES = [1, 63, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]

TABLES = {
    "hash_L16_T19": dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048, gridtype='hash'),
    "hash_L4": dict(input_dim=3, num_levels=4, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048, gridtype='hash'),
    "tiled_L16_T19_8192": dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=8192, gridtype='tiled'),
    # 2^21 entries of 4 bytes per level: more than an XCD's 4 MiB L2 -> the tiles are dealt to the XCDs in contiguous runs
    "tiled_L4_T21": dict(input_dim=3, num_levels=4, level_dim=2, base_resolution=128, log2_hashmap_size=21, desired_resolution=1024, gridtype='tiled'),
}
_built = {}


def table(name):
    if name not in _built:
        from customnerf_amd.gridencoder import GridEncoder
        enc = GridEncoder(**TABLES[name]).cuda()
        g = torch.Generator(device="cuda").manual_seed(3)
        with torch.no_grad():
            enc.embeddings.copy_(torch.rand(enc.embeddings.shape, generator=g, device="cuda") * 2 - 1)
        _built[name] = enc
    return _built[name]


def samples(B, seed):
    """[B, 3] in [0, 1] with the corners, the centre and two out-of-range rows among the first ones (as far as B goes)"""
    rng = np.random.default_rng(seed)
    x = rng.random((max(B, 8), 3)).astype(np.float32)
    x[0] = 0.0
    x[1] = 1.0
    x[2, 0] = -0.01
    x[3, 2] = 1.001
    x[4] = 0.5
    x[5] = (1.0, 0.0, 1.0)
    # a ray's worth of neighbours in space, so that lanes share table rows
    if B > 200:
        x[64:128] = x[64] + np.linspace(0, 0.01, 64, dtype=np.float32)[:, None]
    return torch.from_numpy(np.ascontiguousarray(x[:B])).cuda()


def gather(enc, x, traversal, row0, pad, max_level=None, half=True, fill=7.0):
    """-> [L, row0 + B + pad, 2] buffer pre-filled with `fill`, rows row0 .. row0 + B written by the gather"""
    from customnerf_amd._lib import lib, ptr, stream, check, dtype_id
    tab = enc.half_table() if half else enc.embeddings.detach()
    B, L, C = x.shape[0], enc.num_levels, enc.level_dim
    P = row0 + B + pad
    out = torch.full((L, P, C), fill, dtype=tab.dtype, device="cuda")
    dst = out.data_ptr() + row0 * C * out.element_size()
    check(lib.cnerf_grid_encode_forward_ordered(ptr(x), ptr(tab), enc._offsets_host.ctypes.data, dst, B, 3, C, L, L if max_level is None else max_level,
                                                float(np.log2(enc.per_level_scale)), int(enc.base_resolution), None, enc.gridtype_id, int(enc.align_corners),
                                                enc.interp_id, dtype_id(tab), P, traversal, stream()), "grid_encode_forward_ordered")
    return out


# The XCD-contiguous assignment maps workgroup 8 k + x to tile first(x) + k, XCD x owning q + 1 tiles if x < r, else q (q, r = tiles / 8, tiles % 8).
# Up to 8 tiles that is the identity, so the table that takes it also gets more than 8 tiles: 9 (q = 1, r = 1), 12 with a ragged last one
# (q = 1, r = 4) and 16 (q = 2, r = 0).  A tile skipped or taken twice leaves rows at the fill value or differing from level-major.
XCD_SIZES = [8 * TILE + 1, 11 * TILE + 17, 16 * TILE]
CASES = [(n, B) for n in TABLES for B in SIZES] + [("tiled_L4_T21", B) for B in XCD_SIZES] + [("hash_L16_T19", XCD_SIZES[1])]


@pytest.mark.parametrize("name,B", CASES, ids=[f"{n}-{B}" for n, B in CASES])
def test_tile_shapes_match_level_major(name, B):
    """every batch size around the tile (and, for the XCD-contiguous tiles, beyond eight tiles), at a row offset into a larger buffer
    (out_level_stride > B): equal bytes, nothing written outside the rows"""
    enc = table(name)
    x = samples(B, seed=B)
    row0, pad = 3, 5
    ref = gather(enc, x, 0, row0, pad)
    got = gather(enc, x, 1, row0, pad)
    assert torch.equal(ref.view(torch.int16), got.view(torch.int16))
    assert torch.all(got[:, :row0] == 7.0) and torch.all(got[:, row0 + B:] == 7.0)
    assert not torch.isnan(got.float()).any()
    if B > 4:
        assert torch.all(got[:, row0 + 2] == 0) and torch.all(got[:, row0 + 3] == 0)          # out of range -> zero features
        assert float(got[:, row0 + 4].float().abs().max()) > 0                                 # and an inside sample is not


@pytest.mark.parametrize("name", ["hash_L16_T19", "tiled_L4_T21"])
def test_max_level_below_L(name):
    """max_level < L: the levels above it stay untouched by both forms"""
    enc = table(name)
    x = samples(TILE + 1, seed=11)
    ml = enc.num_levels - 1
    ref = gather(enc, x, 0, 0, 2, max_level=ml)
    got = gather(enc, x, 1, 0, 2, max_level=ml)
    assert torch.equal(ref.view(torch.int16), got.view(torch.int16))
    assert torch.all(got[ml:] == 7.0) and not torch.all(got[ml - 1] == 7.0)


def test_other_tables_ignore_the_switch():
    """a float32 table, and an fp16 table the specialised kernel does not take (4-entry levels): traversal 1 runs the generic kernel"""
    x = samples(TILE + 1, seed=5)
    enc = table("hash_L4")
    assert torch.equal(gather(enc, x, 0, 1, 1, half=False), gather(enc, x, 1, 1, 1, half=False))
    from customnerf_amd.gridencoder import GridEncoder
    tiny = GridEncoder(input_dim=3, num_levels=4, level_dim=2, base_resolution=8, log2_hashmap_size=2, per_level_scale=1.6, gridtype='hash').cuda()
    with torch.no_grad():
        tiny.embeddings.uniform_(-1, 1)
    a, b = gather(tiny, x, 0, 1, 1), gather(tiny, x, 1, 1, 1)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
