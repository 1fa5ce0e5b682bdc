"""Float64 NumPy restatement of the image scores of cnerf_image_metrics (include/customnerf_hip.h), written from the definition there and
not from the kernel: every window is formed explicitly from the image (sliding_window_view), no tiles, no staging.

    quantize(v)      floor(clamp(v, 0, 1) * 255) / 255 in float32
    ssim_map(a, b)   [B, H - 10, W - 10, C] float64: Wang et al. 2004, L = 1, K1 = 0.01, K2 = 0.03, 11-tap Gaussian window of sigma 1.5 with
                     float64 weights normalised to sum 1, separable (rows first), valid region only, population moments
    metrics(...)     per image: mse, l1, psnr, ssim, n_pixels, n_windows (and the map), with the mask rules: a pixel counts when its mask
                     value is nonzero, a window when its centre pixel does; nothing counted -> nan and a count of 0
"""
import numpy as np

TAPS = 11
SIGMA = 1.5
K1, K2 = 0.01, 0.03


def window():
    d = np.arange(TAPS, dtype=np.float64) - TAPS // 2
    g = np.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def quantize(v):
    v = np.asarray(v).astype(np.float32)
    return (np.floor(np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)) / np.float32(255)).astype(np.float32)


def _blur(x):
    """[B, H, W, C] float64 -> [B, H - 10, W - 10, C]: the window along W, then along H, valid positions only"""
    g = window()
    rows = np.lib.stride_tricks.sliding_window_view(x, TAPS, axis=2)            # [B, H, W - 10, C, 11]
    h = np.zeros(rows.shape[:-1], np.float64)
    for k in range(TAPS):
        h = h + g[k] * rows[..., k]
    cols = np.lib.stride_tricks.sliding_window_view(h, TAPS, axis=1)            # [B, H - 10, W - 10, C, 11]
    out = np.zeros(cols.shape[:-1], np.float64)
    for k in range(TAPS):
        out = out + g[k] * cols[..., k]
    return out


def ssim_map(a, b):
    a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    if a.ndim != 4 or a.shape != b.shape or a.shape[1] < TAPS or a.shape[2] < TAPS:
        raise ValueError(f"ssim_map: [B, H >= 11, W >= 11, C] pairs, got {a.shape} and {b.shape}")
    c1, c2 = K1 * K1, K2 * K2
    mu_a, mu_b = _blur(a), _blur(b)
    var_a = _blur(a * a) - mu_a * mu_a
    var_b = _blur(b * b) - mu_b * mu_b
    cov = _blur(a * b) - mu_a * mu_b
    return ((2.0 * (mu_a * mu_b) + c1) * (2.0 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))


def metrics(pred, target, mask=None, quantize_images=False):
    """pred, target [B, H, W, C] (float16 / float32 arrays), mask None or [B, H, W] -> dict of [B] float64 arrays + 'ssim_map'"""
    if quantize_images:
        pred, target = quantize(pred), quantize(target)
    a, b = np.asarray(pred).astype(np.float64), np.asarray(target).astype(np.float64)
    B, H, W, C = a.shape
    smap = ssim_map(a, b)
    m = np.ones((B, H, W), bool) if mask is None else (np.asarray(mask) != 0)
    centre = m[:, TAPS // 2:H - TAPS // 2, TAPS // 2:W - TAPS // 2]
    d = a - b
    out = {k: np.zeros(B, np.float64) for k in ("mse", "l1", "psnr", "ssim", "n_pixels", "n_windows")}
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(B):
            n = float(m[i].sum() * C)
            nw = float(centre[i].sum() * C)
            out["n_pixels"][i], out["n_windows"][i] = n, nw
            out["mse"][i] = np.float64((d[i][m[i]] ** 2).sum()) / n
            out["l1"][i] = np.float64(np.abs(d[i][m[i]]).sum()) / n
            out["psnr"][i] = 10.0 * np.log10(np.float64(1.0) / out["mse"][i])
            out["ssim"][i] = np.float64(smap[i][centre[i]].sum()) / nw
    out["ssim_map"] = smap
    return out
