"""Float64 torch restatement of the SSIM of include/customnerf_hip.h and of its gradient with respect to pred, written from the definition
and not from the kernels: a valid-region separable window (rows first, taps added in order, exactly the operations of
tests/ssim_restatement.py, so the two maps are the same bits), the window-centre mask rule, and torch.autograd for the gradient.

    ssim_map(a, b)             [B, H - 10, W - 10, C] float64 tensor (differentiable)
    centre(mask, B, H, W)      [B, H - 10, W - 10] bool: which windows count (all of them without a mask)
    ssim_and_grad(p, t, mask)  (ssim [B], d ssim_b / d pred [B, H, W, C]) float64 by autograd; an image with no counted window: nan and zeros
    closed_form_grad(...)      the same gradient from the three coefficient maps and explicit transposed window filters (the header's formulas):
                               what the kernels implement, restated without tiles
"""
import numpy as np
import torch

import ssim_restatement as R

TAPS = R.TAPS
C1, C2 = R.K1 * R.K1, R.K2 * R.K2


def _t64(x):
    if torch.is_tensor(x):
        return x.detach().cpu().to(torch.float64)
    return torch.from_numpy(np.asarray(x).astype(np.float64))


def blur(x):
    """[B, H, W, C] float64 -> [B, H - 10, W - 10, C]: the window along W, then along H, valid positions only, taps added in order"""
    g = R.window()
    Wv, Hv = x.shape[2] - (TAPS - 1), x.shape[1] - (TAPS - 1)
    h = torch.zeros(x.shape[0], x.shape[1], Wv, x.shape[3], dtype=torch.float64)
    for k in range(TAPS):
        h = h + float(g[k]) * x[:, :, k:k + Wv, :]
    out = torch.zeros(x.shape[0], Hv, Wv, x.shape[3], dtype=torch.float64)
    for k in range(TAPS):
        out = out + float(g[k]) * h[:, k:k + Hv, :, :]
    return out


def _pieces(a, b):
    mu_a, mu_b = blur(a), blur(b)
    var_a = blur(a * a) - mu_a * mu_a
    var_b = blur(b * b) - mu_b * mu_b
    cov = blur(a * b) - mu_a * mu_b
    return mu_a, mu_b, 2.0 * (mu_a * mu_b) + C1, 2.0 * cov + C2, mu_a * mu_a + mu_b * mu_b + C1, var_a + var_b + C2


def ssim_map(a, b):
    _, _, A1, A2, B1, B2 = _pieces(a, b)
    return (A1 * A2) / (B1 * B2)


def centre(mask, B, H, W):
    m = torch.ones(B, H, W, dtype=torch.bool) if mask is None else (_t64(mask) != 0)
    return m[:, TAPS // 2:H - TAPS // 2, TAPS // 2:W - TAPS // 2]


def ssim_of(pred64, target64, mask=None):
    """differentiable per-image SSIM [B] of float64 tensors (nan where no window counts), and the counts [B]"""
    B, H, W, C = pred64.shape
    smap = ssim_map(pred64, target64)
    cen = centre(mask, B, H, W)
    n = cen.reshape(B, -1).sum(1).to(torch.float64) * C
    total = (smap * cen[..., None].to(torch.float64)).reshape(B, -1).sum(1)
    return total / n, n


def ssim_and_grad(pred, target, mask=None):
    a = _t64(pred).requires_grad_(True)
    b = _t64(target)
    s, n = ssim_of(a, b, mask)
    grad = torch.zeros_like(a)
    for i in range(a.shape[0]):
        if n[i] > 0:
            grad[i] = torch.autograd.grad(s[i], a, retain_graph=True)[0][i]
    return s.detach(), grad


def closed_form_grad(pred, target, mask=None):
    a, b = _t64(pred), _t64(target)
    B, H, W, C = a.shape
    Hv, Wv = H - (TAPS - 1), W - (TAPS - 1)
    mu_a, mu_b, A1, A2, B1, B2 = _pieces(a, b)
    s = (A1 * A2) / (B1 * B2)
    cen = centre(mask, B, H, W)
    n = cen.reshape(B, -1).sum(1).to(torch.float64) * C
    gw = torch.where(n > 0, 1.0 / n, torch.zeros_like(n)).reshape(B, 1, 1, 1) * cen[..., None].to(torch.float64)     # g_p
    d_ab = 2.0 * A1 / (B1 * B2)
    d_aa = -s / B2
    d_mu = 2.0 * mu_b * (A2 - A1) / (B1 * B2) + 2.0 * mu_a * s * (1.0 / B2 - 1.0 / B1)
    g = R.window()

    def transposed(m):                                           # [B, Hv, Wv, C] -> [B, H, W, C], zeros outside
        out = torch.zeros(B, H, W, C, dtype=torch.float64)
        for k in range(TAPS):
            for l in range(TAPS):
                out[:, k:k + Hv, l:l + Wv, :] += float(g[k] * g[l]) * m
        return out
    return transposed(gw * d_mu) + 2.0 * a * transposed(gw * d_aa) + b * transposed(gw * d_ab)
