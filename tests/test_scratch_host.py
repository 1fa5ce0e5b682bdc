"""_lib.ScratchCache, the one owner of the package's grow-on-demand device workspaces, on CPU tensors with plain string keys (no stream, no
GPU), and the parameters the six module-level caches give it."""
import importlib
import weakref

import pytest
import torch

from customnerf_amd._lib import ScratchCache, scratch_generation

CPU = torch.device("cpu")


def test_releasing_cache_grows_with_headroom_and_bumps_the_generation():
    c = ScratchCache(factor=1.25, pad=256)
    gen = scratch_generation()
    a = c.reserve("k", 1000, CPU)
    assert a.numel() == 1506 and a.dtype == torch.uint8 and scratch_generation() == gen + 1
    for n in (1000, 1, 1506):
        assert c.reserve("k", n, CPU) is a
    assert scratch_generation() == gen + 1
    b = c.reserve("k", 1507, CPU)
    assert b is not a and b.numel() == int(1507 * 1.25) + 256 and scratch_generation() == gen + 2
    assert c["k"] is b and list(c.values()) == [b] and not c.retired
    ref = weakref.ref(a)
    del a
    assert ref() is None                                     # nothing in the cache keeps the outgrown buffer


def test_shrinking_cache_releases_an_oversized_buffer():
    c = ScratchCache(dtype=torch.float32, shrink=4)
    big = c.reserve("k", 4096 * 1024 * 2, CPU).numel()
    assert big == 4096 * 1024 * 2 and c["k"].dtype == torch.float32
    gen = scratch_generation()
    assert c.reserve("k", big // 4, CPU).numel() == big      # a quarter of what is held: kept
    assert scratch_generation() == gen
    c.reserve("k", 64 * 1024 * 2, CPU)
    assert c["k"].numel() < big // 4 + 1 and c["k"].numel() >= 64 * 1024 * 2 and scratch_generation() == gen + 1


def test_retiring_cache_keeps_outgrown_buffers_and_the_generation():
    c = ScratchCache(floor=64, retire=True)
    gen = scratch_generation()
    a = c.reserve("k", 10, CPU)
    assert a.numel() == 64 and c.reserve("k", 64, CPU) is a and not c.retired
    b = c.reserve("k", 100, CPU)
    assert b is not a and b.numel() == 100 and c["k"] is b
    assert len(c.retired) == 1 and c.retired[0] is a and a.numel() == 64      # still allocated
    assert scratch_generation() == gen


def test_drop_bumps_the_generation_only_for_a_held_key():
    c = ScratchCache()
    c.reserve("k", 8, CPU)
    gen = scratch_generation()
    c.drop("absent")
    assert scratch_generation() == gen and "k" in c
    c.drop("k")
    assert scratch_generation() == gen + 1 and "k" not in c and not c
    c.drop("k")
    assert scratch_generation() == gen + 1


def test_two_keys_are_independent():
    c = ScratchCache(factor=1.25, pad=256)
    a, b = c.reserve("a", 100, CPU), c.reserve("b", 5000, CPU)
    assert a is not b and (a.numel(), b.numel()) == (381, 6506) and len(c) == 2
    a2 = c.reserve("a", 1000, CPU)
    assert a2 is not a and c["b"] is b and c.reserve("b", 5000, CPU) is b
    c.drop("a")
    assert list(c) == ["b"]


# (module, how to reach the cache) -> (factor, pad, floor, dtype, shrink, retire)
CACHES = [
    ("customnerf_amd.field", lambda m: m._WS, (1.1, 256, 0, torch.uint8, None, False)),
    ("customnerf_amd.mlp", lambda m: m._WS, (1.1, 256, 0, torch.uint8, None, False)),
    ("customnerf_amd.gridencoder.grid", lambda m: m._WS_CACHE, (1.25, 256, 0, torch.uint8, None, False)),
    ("customnerf_amd.raymarching.raymarching", lambda m: m._HITS, (1, 0, 0, torch.float32, 4, False)),
    ("customnerf_amd.sd.ops", lambda m: m._WS, (1, 0, 64 << 20, torch.uint8, None, True)),
]


@pytest.mark.parametrize("module,get,want", CACHES, ids=["field", "mlp", "grid", "hits", "sd_ops"])
def test_module_caches_carry_their_parameters(module, get, want):
    mod = importlib.import_module(module)
    c = get(mod)
    assert isinstance(c, ScratchCache)
    assert (c.factor, c.pad, c.floor, c.dtype, c.shrink, c.retire) == want
    if module == "customnerf_amd.sd.ops":
        assert mod._WS_RETIRED is c.retired
