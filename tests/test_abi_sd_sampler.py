"""CPU: argument validation of the image-sampling entry points (csrc/sd_sample.hip) — every rejected call returns CNERF_EINVAL
before anything touches the device.  No launch is issued here."""
import ctypes

import pytest

EINVAL = -1
ONE = ctypes.c_void_p(1 << 20)            # non-NULL, 16-byte aligned dummy: never dereferenced on these paths


def _ddim(**over):
    from customnerf_amd._lib import lib
    a = dict(eps=ONE, ld_eps=8, latents=ONE, ab_t=0.5, ab_prev=0.6, g=7.5, mode=0, pairs=1, pixels=35, latents_out=ONE, x0_out=ONE, unet_in=ONE)
    a.update(over)
    return lib.cnerf_sd_ddim_step(a["eps"], a["ld_eps"], a["latents"], a["ab_t"], a["ab_prev"], a["g"], a["mode"], a["pairs"], a["pixels"], a["latents_out"],
                                  a["x0_out"], a["unet_in"], None)


@pytest.mark.parametrize("over", [
    dict(eps=None), dict(latents=None), dict(latents_out=None, x0_out=None, unet_in=None),         # NULL inputs; no output at all
    dict(pixels=0), dict(pairs=0), dict(ld_eps=3), dict(ld_eps=0),
    dict(ab_t=0.0), dict(ab_t=-0.1), dict(ab_t=1.0001), dict(ab_t=float("nan")),
    dict(ab_prev=0.0), dict(ab_prev=1.5), dict(ab_prev=float("nan")),
    dict(mode=2), dict(mode=-1),
    dict(unet_in=ctypes.c_void_p((1 << 20) + 8)),                                                  # the half output is written 16 bytes at a time
    dict(pairs=1 << 16, pixels=1 << 16),                                                           # element index past 32 bits
])
def test_ddim_step_rejects(over):
    assert _ddim(**over) == EINVAL


def test_decoder_glue_rejects():
    from customnerf_amd._lib import lib
    din, dout = lib.cnerf_sd_decoder_input, lib.cnerf_sd_decoder_output
    for args in ((None, 1, 64, 0.18215, ONE, ONE), (ONE, 1, 64, 0.18215, None, ONE), (ONE, 1, 64, 0.18215, ONE, None),
                 (ONE, 0, 64, 0.18215, ONE, ONE), (ONE, 1, 0, 0.18215, ONE, ONE), (ONE, 1, 64, 0.0, ONE, ONE), (ONE, 1, 64, float("nan"), ONE, ONE),
                 (ONE, 1 << 14, 1 << 14, 0.18215, ONE, ONE), (ONE, 1, 64, 0.18215, ONE, ctypes.c_void_p((1 << 20) + 2))):
        assert din(*args, None) == EINVAL, args
    for args in ((None, 8, 1, 64, ONE, ONE), (ONE, 8, 1, 64, None, None), (ONE, 2, 1, 64, ONE, ONE), (ONE, 8, 0, 64, ONE, ONE), (ONE, 8, 1, 0, ONE, ONE),
                 (ONE, 8, 1 << 16, 1 << 16, ONE, ONE)):
        assert dout(*args, None) == EINVAL, args
