"""Restatement in torch of the two regularisers of the ray weights ("Ray regularisers"), written from their definitions:
the distortion loss as the literal O(S^2) double sum, the transmittance as a cumprod, gradients from torch.autograd.  float64 by default;
dtype=torch.float32 is the same program in float32, the yardstick for what float32 arithmetic alone costs.  Nothing here is shared with the
kernels: no prefix sums, no closed-form gradient (those are stated separately below, for the host tests that compare the two).

Per ray and composite variant v (0 all, 1 edit region, 2 background), sigma [N, S], rgbc [N, S, 4], z [N, S] non-decreasing:
  delta_i = z_{i+1} - z_i, the last one (far - near) / num_steps;   s_v = sigma * (1 | e | 1 - e),  e = sigmoid((conf - thr) * 100) | conf > 0.5
  alpha = 1 - exp(-delta s_v),  T_i = prod_{j<i} (1 - alpha_j + 1e-15),  w = alpha T
  L = far - near,  d = delta / L,  m = (z - near) / L + d / 2
  distortion = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i
  entropy    = -sum_i p_i log(p_i + 1e-10),  p = w / (W + 1e-10),  W = sum w;   reported only where W > min_opacity (a constant gate), else 0
A ray with !(far > near) has both losses 0 and no gradient."""
import numpy as np
import torch

D = torch.float64


def _inputs(sigma, rgbc, z, nears, fars, dtype):
    N, S = z.shape
    z, nears, fars = (torch.as_tensor(a).detach().cpu().to(dtype) for a in (z, nears, fars))
    return sigma.reshape(N, S), rgbc.reshape(N, S, 4), z, nears.reshape(N, 1), fars.reshape(N, 1)


def weights(sigma, conf, z, nears, fars, num_steps, soft, thr, v, detach_bg, dtype):
    """-> w [N, S], alpha, T, delta, hit [N, 1], L (1 where the ray misses, so that nothing divides by zero there)"""
    hit = fars > nears
    L = torch.where(hit, fars - nears, torch.ones_like(fars))
    sd = torch.where(hit, (fars - nears) / num_steps, torch.zeros_like(fars))
    delta = torch.cat([z[:, 1:] - z[:, :-1], sd], 1)
    thr = float(np.float32(thr))                                       # the kernel receives the threshold as a float
    e = torch.sigmoid((conf - thr) * 100) if soft else (conf > 0.5).to(dtype)
    s = sigma
    if v == 0 and detach_bg:                                           # the `all` composite: no density gradient outside the edit region
        s = torch.where(conf >= 0.5, sigma, sigma.detach())
    s = s * (1.0 if v == 0 else (e if v == 1 else 1 - e))
    alpha = 1 - torch.exp(-delta * s)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha + 1e-15], -1), -1)[:, :-1]
    return alpha * T, alpha, T, delta, hit, L


def regularizers(sigma, rgbc, z, nears, fars, num_steps, soft, thr, detach_bg=False, variants=(0, 1, 2), min_opacity=0.1, dtype=D):
    """-> [3, N, 2] (distortion, entropy), differentiable in sigma and rgbc; rows of variants that were not asked for are zeros"""
    sigma, rgbc, z, nears, fars = _inputs(sigma, rgbc, z, nears, fars, dtype)
    N, S = z.shape
    conf = rgbc[..., 3]
    out = []
    for v in range(3):
        if v not in variants:
            out.append(torch.zeros(N, 2, dtype=dtype))
            continue
        w, _, _, delta, hit, L = weights(sigma, conf, z, nears, fars, num_steps, soft, thr, v, detach_bg, dtype)
        d = delta / L
        m = (z - nears) / L + d / 2
        dist = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2)) + (w * w * d).sum(1) / 3
        W = w.sum(1, keepdim=True)
        p = w / (W + 1e-10)
        ent = -(p * torch.log(p + 1e-10)).sum(1)
        ent = torch.where(W.detach()[:, 0] > float(np.float32(min_opacity)), ent, torch.zeros_like(ent))
        h = hit[:, 0]
        out.append(torch.stack([torch.where(h, dist, torch.zeros_like(dist)), torch.where(h, ent, torch.zeros_like(ent))], -1))
    return torch.stack(out)


def regularizers_with_grads(sigma, rgbc, z, nears, fars, num_steps, soft, thr, g_reg, detach_bg=False, variants=(0, 1, 2), min_opacity=0.1, dtype=D):
    """-> out [3, N, 2], d sum(out * g_reg) / d sigma [N, S], / d rgbc [N, S, 4] (autograd)"""
    N, S = z.shape
    s = torch.as_tensor(sigma).detach().cpu().to(dtype).reshape(N, S).requires_grad_(True)
    c = torch.as_tensor(rgbc).detach().cpu().to(dtype).reshape(N, S, 4).requires_grad_(True)
    g = torch.as_tensor(g_reg).detach().cpu().to(dtype)
    out = regularizers(s, c, z, nears, fars, num_steps, soft, thr, detach_bg, variants, min_opacity, dtype)
    ((s * 0).sum() + (c * 0).sum() + (out * g).sum()).backward()
    return out.detach(), s.grad, c.grad


# ------------------------------------------------------------------------------------------------ the forms the kernels implement
# (host tests only: tests/test_ray_reg_host.py checks them against the definitions above; the GPU tests never call them)
def distortion_prefix(w, delta, L):
    """the distortion by prefix sums, O(S): with ascending samples m_l - m_{l-1} = (d_{l-1} + d_l) / 2 =: dm_l >= 0 and
    A_k = sum_{j<k} w_j (m_k - m_j) = sum_{l<=k} W_{<l} dm_l, so sum_i sum_j w_i w_j |m_i - m_j| = 2 sum_i w_i A_i.
    -> distortion [N], dD/dw [N, S] = 2 (A_k + B_k) + (2/3) w_k d_k with B_k = sum_{l>k} W_{>=l} dm_l"""
    d = delta / L
    dm = torch.cat([torch.zeros_like(d[:, :1]), (d[:, :-1] + d[:, 1:]) / 2], 1)
    Wlt = torch.cumsum(w, 1) - w
    A = torch.cumsum(Wlt * dm, 1)
    Wge = w.sum(1, keepdim=True) - Wlt
    E = torch.cumsum(Wge * dm, 1)
    B = E[:, -1:] - E
    return (2 * w * A).sum(1) + (w * w * d).sum(1) / 3, 2 * (A + B) + (2.0 / 3.0) * w * d


def closed_form_grads(sigma, rgbc, z, nears, fars, num_steps, soft, thr, g_reg, detach_bg=False, variants=(0, 1, 2), min_opacity=0.1, dtype=D):
    """d sum(out * g_reg) / d sigma, / d conf from the closed forms: G = dL/dw per variant, then dL/dalpha_i = G_i T_i - (sum_{k>i} G_k w_k) / q_i,
    ds_v = dalpha delta (1 - alpha), g_sigma += ds_v scale, g_conf = +-ds_v sigma 100 e (1 - e) under the soft mask"""
    sigma, rgbc, z, nears, fars = _inputs(torch.as_tensor(sigma).detach().cpu().to(dtype), torch.as_tensor(rgbc).detach().cpu().to(dtype), z, nears, fars, dtype)
    g_reg = torch.as_tensor(g_reg).detach().cpu().to(dtype)
    conf = rgbc[..., 3]
    thr32 = float(np.float32(thr))
    e = torch.sigmoid((conf - thr32) * 100) if soft else (conf > 0.5).to(dtype)
    g_sigma, g_conf = torch.zeros_like(sigma), torch.zeros_like(sigma)
    for v in variants:
        w, alpha, T, delta, hit, L = weights(sigma, conf, z, nears, fars, num_steps, soft, thr, v, False, dtype)
        _, GD = distortion_prefix(w, delta, L)
        W = w.sum(1, keepdim=True)
        p = w / (W + 1e-10)
        h = -(torch.log(p + 1e-10) + p / (p + 1e-10))
        GH = (h - (p * h).sum(1, keepdim=True)) / (W + 1e-10)
        GH = torch.where(W > float(np.float32(min_opacity)), GH, torch.zeros_like(GH))
        G = g_reg[v, :, 0:1] * GD + g_reg[v, :, 1:2] * GH
        Gw = G * w
        suffix = Gw.sum(1, keepdim=True) - torch.cumsum(Gw, 1)
        dalpha = G * T - suffix / (1 - alpha + 1e-15)
        ds = torch.where(hit, dalpha * delta * (1 - alpha), torch.zeros_like(w))
        scale = torch.ones_like(e) if v == 0 else (e if v == 1 else 1 - e)
        keep = (conf >= 0.5) if (v == 0 and detach_bg) else torch.ones_like(conf, dtype=torch.bool)
        g_sigma = g_sigma + torch.where(keep, ds * scale, torch.zeros_like(ds))
        if soft and v > 0:
            g_conf = g_conf + (1 if v == 1 else -1) * ds * sigma * 100 * e * (1 - e)
    return g_sigma, g_conf
