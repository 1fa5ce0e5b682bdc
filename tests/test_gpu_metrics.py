"""GPU: cnerf_image_metrics (csrc/metrics.hip) through customnerf_amd.metrics against tests/ssim_restatement.py, the float64 NumPy
restatement of the definition in include/customnerf_hip.h (itself checked in tests/test_metrics_host.py).

Tolerances, derived, not measured.  The kernel and the restatement both form every window moment as a 22-term float64 sum of products of
weights <= 1 and values in [0, 1] (11 taps along a row, 11 along a column), in different orders: each is within 22 * 2^-53 = 2.4e-15 of the
exact value.  The SSIM quotient divides by at least C1 * C2 with a numerator of that size, and its sensitivity to a moment is at most
~2 / C2 = 2.2e3: the maps agree to 1e-9 absolute with a wide margin.  The map is STORED as float32, so the stored value is compared with
the restatement rounded to float32, one ulp allowed (a 1e-9 difference can straddle a rounding boundary, never two).  The per-image
numbers are float64 sums of at most ~2e4 such terms in another order: 1e-12 relative.
T = 32 is the kernel's tile edge: the shapes below are the ones at which a tile kernel changes path."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ssim_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

T = 32
SHAPES = [(11, 11), (11, 12), (12, 11), (T + 10, T + 10), (T + 11, T + 10), (T + 10, T + 11), (2 * T + 11, 11), (43, 75)]
KEYS = ("mse", "l1", "ssim")


def _run(pred, target, mask=None, quantize=False, dtype=torch.float32):
    from customnerf_amd import metrics as M
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = M.image_metrics(dev(pred).to(dtype), dev(target).to(dtype), mask=dev(mask), quantize=quantize, want_map=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, want, what=""):
    """the tolerances of the module docstring; counts exact; nan where the restatement is nan"""
    assert got["ssim_map"].dtype == np.float32 and got["ssim_map"].shape == want["ssim_map"].shape
    ref32 = want["ssim_map"].astype(np.float32)
    ulps = np.abs(got["ssim_map"].astype(np.float64) - ref32.astype(np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64)
    err = np.abs(got["ssim_map"].astype(np.float64) - want["ssim_map"]).max()
    print(f"{what}: map max |diff| to float64 {err:.3e} (float32 storage), max ulps to the rounded restatement {ulps.max():.2f}")
    assert ulps.max() <= 1.0, what
    for k in ("n_pixels", "n_windows"):
        assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in KEYS + ("psnr",):
        g, w = got[k], want[k]
        assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(w)), (what, k, g, w)
        ok = ~np.isnan(w)
        rel = np.abs(g[ok] - w[ok]) / np.maximum(np.abs(w[ok]), 1e-300) if k != "psnr" else np.abs(g[ok] - w[ok]) / np.maximum(np.abs(w[ok]), 1.0)
        rel = np.where(g[ok] == w[ok], 0.0, rel)                                             # (inf == inf)
        print(f"{what}: {k} max relative diff {rel.max() if rel.size else 0.0:.3e}")
        assert np.all(rel <= 1e-12), (what, k, g, w)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H, W", SHAPES)
def test_shapes_against_restatement(H, W, C):
    rng = np.random.default_rng(H * 1000 + W * 10 + C)
    pred = rng.random((2, H, W, C)).astype(np.float32)                                       # B = 2, different content per image
    target = np.clip(pred + 0.2 * rng.standard_normal((2, H, W, C)), 0, 1).astype(np.float32)
    target[1] = rng.random((H, W, C)).astype(np.float32)
    want = R.metrics(pred, target)
    assert want["ssim"][0] != want["ssim"][1]
    _check(_run(pred, target), want, f"{H}x{W}x{C}")


def _separating_inputs():
    rng = np.random.default_rng(5)
    H, W = 43, 75
    flat = (np.full((1, H, W, 3), 1.0, np.float32), np.full((1, H, W, 3), 0.9, np.float32))
    noise = tuple((0.7 + 1e-3 * rng.standard_normal((1, H, W, 3))).astype(np.float32) for _ in range(2))
    x = np.arange(W)
    step = tuple(np.broadcast_to(np.where(x < W // 2 + s, 0.1, 0.95).astype(np.float32)[None, None, :, None], (1, H, W, 3)).copy() for s in (0, 1))
    return {"flat_1.0_0.9": flat, "0.7_plus_1e-3_noise": noise, "step_offset_by_one_column": step}


@pytest.mark.parametrize("name", ["flat_1.0_0.9", "0.7_plus_1e-3_noise", "step_offset_by_one_column"])
def test_inputs_that_separate_float64_moments_from_float32(name):
    """a float32 restatement of the plain formula misses these by ~1e-4; the tolerances are the ones above"""
    a, b = _separating_inputs()[name]
    want = R.metrics(a, b)
    got = _run(a, b)
    if name.startswith("flat"):
        assert abs(want["ssim"][0] - (2 * 0.9 + 1e-4) / (1 + float(np.float32(0.9)) ** 2 + 1e-4)) < 1e-7
    _check(got, want, name)


def test_halo_single_bright_pixel_across_four_tiles():
    """75 x 75: 65 x 65 windows in 3 x 3 tiles.  Image 0: pixel (37, 37) lies in the windows [27, 37]^2, which meet four tiles at 32.  Image 1:
    pixel (2, 70) near the corner: its footprint is clipped to the windows rows [0, 2] x columns [60, 64]."""
    rng = np.random.default_rng(9)
    H = W = 2 * T + 11
    target = rng.random((2, H, W, 1)).astype(np.float32)
    dark = np.zeros((2, H, W, 1), np.float32)
    lit = dark.copy()
    lit[0, 37, 37, 0] = 1.0
    lit[1, 2, 70, 0] = 1.0
    got_dark, got_lit = _run(dark, target), _run(lit, target)
    _check(got_lit, R.metrics(lit, target), "halo")
    changed = got_lit["ssim_map"] != got_dark["ssim_map"]
    want = np.zeros_like(changed)
    want[0, 27:38, 27:38] = True
    want[1, 0:3, 60:65] = True
    assert changed[0].sum() == 121 and changed[1].sum() == 15 and np.array_equal(changed, want)


def test_exact_properties():
    from customnerf_amd import metrics as M
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 43, 75, 3, generator=g).cuda()
    y = torch.rand(2, 43, 75, 3, generator=g).cuda()
    same = M.image_metrics(x, x, want_map=True)
    assert bool((same["ssim"] == 1.0).all()) and bool(torch.isposinf(same["psnr"]).all()) and bool((same["ssim_map"] == 1.0).all())
    assert bool((same["mse"] == 0).all()) and bool((same["l1"] == 0).all())
    one, two = M.image_metrics(x, y, want_map=True), M.image_metrics(x, y, want_map=True)
    for k in one:
        assert torch.equal(one[k], two[k]), k                                                # bit-identical from run to run
    xh, yh = x.half(), y.half()
    h, f = M.image_metrics(xh, yh, want_map=True), M.image_metrics(xh.float(), yh.float(), want_map=True)
    for k in h:
        assert torch.equal(h[k], f[k]), k                                                    # float16 widens exactly
    assert float(M.psnr(x, y)[1]) == float(one["psnr"][1]) and float(M.ssim(x, y)[0]) == float(one["ssim"][0])
    # [H, W, C] is a batch of one; a non-contiguous view is made contiguous
    single = M.image_metrics(x[1], y[1])
    assert single["ssim"].shape == (1,) and float(single["ssim"][0]) == float(one["ssim"][1])
    xt = x.permute(0, 2, 1, 3)
    assert not xt.is_contiguous()
    tr = M.image_metrics(xt, y.permute(0, 2, 1, 3))
    assert torch.equal(tr["mse"], M.image_metrics(xt.contiguous(), y.permute(0, 2, 1, 3).contiguous())["mse"])
    with pytest.raises(ValueError):
        M.image_metrics(x[:, :10], y[:, :10])                                                # H = 10: below one window
    with pytest.raises(ValueError):
        M.image_metrics(x[..., :2], y[..., :2])                                              # C = 2
    with pytest.raises(ValueError):
        M.image_metrics(x, y[:, :20])


def test_masks():
    rng = np.random.default_rng(21)
    H, W = 43, 75
    pred, target = rng.random((3, H, W, 3)).astype(np.float32), rng.random((3, H, W, 3)).astype(np.float32)
    mask = np.zeros((3, H, W), np.float32)
    mask[1, H - 6, W - 6] = 1.0           # one pixel: the centre of the LAST window of the last tile (its far corner)
    mask[2] = (rng.random((H, W)) < 0.4) * rng.integers(1, 4, (H, W))                        # random, nonzero values other than 1 too
    want = R.metrics(pred, target, mask)
    assert want["n_pixels"].tolist()[:2] == [0, 3] and want["n_windows"].tolist()[:2] == [0, 3] and want["n_windows"][2] < want["n_pixels"][2]
    got = _run(pred, target, mask)
    assert np.isnan(got["ssim"][0]) and np.isnan(got["mse"][0]) and np.isnan(got["psnr"][0]) and got["n_pixels"][0] == 0 and got["n_windows"][0] == 0
    _check(got, want, "masks")
    # a masked pixel in the far corner of the IMAGE: counted for the errors by the last tile (which owns the halo strip), centre of no window
    corner = np.zeros((1, H, W), np.float32)
    corner[0, H - 1, W - 1] = 1.0
    want_c = R.metrics(pred[:1], target[:1], corner)
    assert want_c["n_pixels"][0] == 3 and want_c["n_windows"][0] == 0
    _check(_run(pred[:1], target[:1], corner), want_c, "corner")
    # foreground + background = everything
    from customnerf_amd import metrics as M
    p, t, m = (torch.from_numpy(a).cuda() for a in (pred, target, (mask != 0).astype(np.float32)))
    fg, bg, al = M.image_metrics(p, t, m), M.image_metrics(p, t, 1 - m), M.image_metrics(p, t)
    assert torch.equal(fg["n_pixels"] + bg["n_pixels"], al["n_pixels"]) and torch.equal(fg["n_windows"] + bg["n_windows"], al["n_windows"])
    assert bool((al["n_pixels"] == H * W * 3).all())


def test_quantize_truncates():
    rng = np.random.default_rng(33)
    H, W = 43, 44
    pred = (rng.random((1, H, W, 3)) * 1.2 - 0.1).astype(np.float32)                         # beyond [0, 1] on both sides: the clamp
    target = rng.random((1, H, W, 3)).astype(np.float32)
    pred[0, 0, :4, 0] = [0.999, 1.0, 254.5 / 255, 0.5]
    target[0, 0, :4, 0] = [1.0, 0.999, 1.0, 127.0 / 255]
    want = R.metrics(pred, target, quantize_images=True)
    got = _run(pred, target, quantize=True)
    _check(got, want, "quantize")
    _check(_run(R.quantize(pred), R.quantize(target)), want, "quantized inputs")
    # 0.999 is stored as 254, not rounded to 255: against a constant 1.0 the error is exactly 1 / 255 per pixel
    a, b = np.full((1, 11, 11, 1), 0.999, np.float32), np.ones((1, 11, 11, 1), np.float32)
    q = _run(a, b, quantize=True)
    step = float(np.float32(1) - np.float32(254) / np.float32(255))
    assert abs(q["l1"][0] - step) <= 1e-12 * step and abs(_run(a, b)["l1"][0] - (1 - float(np.float32(0.999)))) <= 1e-15
    h = _run(pred, target, quantize=True, dtype=torch.float16)
    _check(h, R.metrics(pred.astype(np.float16), target.astype(np.float16), quantize_images=True), "quantize float16")


def test_clip_scores():
    """equal to a float64 cosine on the embeddings the same encoders return, to 1e-6 (the embeddings are float32; the cosines are formed in
    float64 on both sides, so only the order of a 64-term sum differs); swapping source and edited negates the directional score"""
    from customnerf_amd import metrics as M
    from customnerf_amd.sd import clip_view as cv
    clip = cv.CLIP("cuda", cfg=cv.CLIP_TINY, seed=2)
    g = torch.Generator().manual_seed(4)
    src, edit = torch.rand(3, 3, 48, 48, generator=g).cuda(), torch.rand(3, 3, 48, 48, generator=g).cuda()
    toks = torch.zeros(2, 77, dtype=torch.int64)
    vocab = cv.CLIP_TINY["vocab_size"]
    for i in range(2):
        toks[i, :5 + i] = torch.randint(1, vocab - 2, (5 + i,), generator=g)
        toks[i, 5 + i] = vocab - 1
    t_src, t_edit = toks[:1].cuda(), toks[1:].cuda()
    out = M.clip_scores(clip, src, edit, t_src, t_edit)
    ei_s, ei_e = clip.encode_img(src).double().cpu().numpy(), clip.encode_img(edit).double().cpu().numpy()
    et_s, et_e = clip.get_text_embeds(t_src).double().cpu().numpy()[0], clip.get_text_embeds(t_edit).double().cpu().numpy()[0]
    cos = lambda a, b: float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
    assert out["clip_text_image"].shape == (3,) and out["clip_text_image"].dtype == torch.float64
    for i in range(3):
        assert abs(float(out["clip_text_image"][i]) - cos(ei_e[i], et_e)) <= 1e-6
        assert abs(float(out["clip_directional"][i]) - cos(ei_e[i] - ei_s[i], et_e - et_s)) <= 1e-6
        assert abs(float(out["clip_directional"][i])) <= 1.0 + 1e-12
    swapped = M.clip_scores(clip, edit, src, t_src, t_edit)
    assert float((swapped["clip_directional"] + out["clip_directional"]).abs().max()) <= 1e-12
    with pytest.raises(RuntimeError):
        M.clip_scores(clip, src, edit, "a bear", "a panda")                                  # no tokenizer injected: token ids
