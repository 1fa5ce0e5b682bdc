"""Float64 restatement of what the `run()` kernels of csrc/render.hip compute (nerf/renderer.py:310-363, 384-474, sample_pdf :21-55, the
reconstruction loss of utils_init_nerf.py:220-234): the stratified coarse samples, the weights -> sample_pdf -> merge chain, the three
weights_sum_i composites (differentiable: gradients come from autograd) and the loss.  Where oracle.torch_oracle is dtype-generic
(sample_pdf, weights_sum_i) it is called on float64 tensors, so this file and the float32 oracle share one definition; what is written out
here is what the oracle builds in float32 (the linspace of run()) or returns no detail of (the conditioning of an inverse-CDF draw).
tests/test_run_restatement_host.py pins it to the reference's own outputs under tests/golden/."""
import numpy as np
import torch

from oracle import torch_oracle as to

D = torch.float64
EPS = 2.0 ** -20                     # 16 float32 ulp of 1.0: the CDF error a float32 evaluation may have (see ill_conditioned)


def f64(x):
    return None if x is None else torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x.detach().cpu()).to(D)


def ulp32(x):
    """spacing of float32 at |x| (elementwise, float64 tensor)"""
    a = np.abs(np.asarray(f64(x).numpy(), np.float64)).astype(np.float32)
    with np.errstate(all="ignore"):
        return torch.from_numpy(np.spacing(a).astype(np.float64))


def sample_coarse(o, d, nears, fars, aabb, T, noise=None):
    """renderer.py:310-322 -> z [N, T], xyz [N, T, 3]"""
    o, d, nears, fars, aabb = f64(o), f64(d), f64(nears).reshape(-1, 1), f64(fars).reshape(-1, 1), f64(aabb)
    z = nears + (fars - nears) * torch.linspace(0.0, 1.0, T, dtype=D)[None]
    if noise is not None:
        z = z + (f64(noise) - 0.5) * ((fars - nears) / T)
    return z, points(o, d, z, aabb)


def points(o, d, z, aabb):
    o, d, z, aabb = f64(o), f64(d), f64(z), f64(aabb)
    return torch.min(torch.max(o[:, None] + d[:, None] * z[..., None], aabb[:3]), aabb[3:])


def coarse_weights(z, sigma, nears, fars, T):
    """renderer.py:336-344 -> weights [N, T], z_vals_mid [N, T - 1]"""
    z, sigma = f64(z), f64(sigma)
    sd = ((f64(fars) - f64(nears)) / T).reshape(-1, 1)
    deltas = torch.cat([z[:, 1:] - z[:, :-1], sd], dim=-1)
    alphas = 1 - torch.exp(-deltas * sigma)
    w = alphas * torch.cumprod(torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-15], dim=-1), dim=-1)[:, :-1]
    return w, z[:, :-1] + 0.5 * deltas[:, :-1]


def sample_pdf_detail(bins, weights, n_samples, det=False, u=None):
    """oracle.torch_oracle.sample_pdf in float64, with what decides how well a draw is conditioned -> dict of [B, n_samples] tensors:
    z (the samples), gap = min_k |u - cdf[k]|, denom_raw = cdf[above] - cdf[below], denom (after the `< 1e-5 -> 1` rule), bins_b, bins_a;
    lo / hi [B] = the row's smallest / largest bin"""
    bins, weights = f64(bins), f64(weights)
    w = weights + 1e-5
    cdf = torch.cumsum(w / torch.sum(w, -1, keepdim=True), -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    if det:
        u = torch.linspace(0. + 0.5 / n_samples, 1. - 0.5 / n_samples, steps=n_samples, dtype=D).expand(cdf.shape[0], n_samples)
    u = f64(u).contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below, above = torch.clamp(inds - 1, min=0), torch.clamp(inds, max=cdf.shape[-1] - 1)
    cdf_b, cdf_a = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bins_b, bins_a = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom_raw = cdf_a - cdf_b
    denom = torch.where(denom_raw < 1e-5, torch.ones_like(denom_raw), denom_raw)
    z = bins_b + (u - cdf_b) / denom * (bins_a - bins_b)
    gap, k = (u[..., None] - cdf[:, None, :]).abs().min(-1)
    return dict(z=z, gap=gap, k=k, bins=bins, denom_raw=denom_raw, denom=denom, bins_b=bins_b, bins_a=bins_a, lo=bins.min(-1).values, hi=bins.max(-1).values, cdf=cdf)


def ill_conditioned(det):
    """A draw whose bin (|u - cdf[k]| < EPS for some k) or whose branch of the `denom < 1e-5` rule (|denom - 1e-5| < EPS) a float32 CDF —
    a scan of at most seven roundings per chunk of 64, one per carried chunk, the total and the divide: under 16 ulp of 1 — may decide the
    other way."""
    return (det["gap"] < EPS) | ((det["denom_raw"] - 1e-5).abs() < EPS)


def near_step(det):
    """Draws within EPS of a CDF step whose two neighbouring bins are clear of the `denom < 1e-5` rule.  They are not rare: the midpoint u
    of the det branch meets a uniform CDF (all-zero weights, a ray that misses the box) ON its steps as a matter of arithmetic —
    u = (2m+1) / (2t) equals k / nb for every draw of (T, t) = (100, 7), for one of (4, 3) and of (128, 127), for 64 bins with 1, 2, 63, 65
    or 200 samples — and two bins behind an opaque sample differ by 1e-11.  So they are not waved through as ill-conditioned.  The
    interpolation is continuous across a step (t = 1 in the bin below and t = 0 in the bin above both give bins[k]): with g = |u - cdf[k]|
    < EPS, the float64 sample is bins[k] -/+ g w_A / d_A in its bin A, and a float32 CDF that puts the draw into the other bin B gives
    bins[k] +/- e w_B / d_B' with e <= EPS and d_B' = d_B (1 +- 2 EPS / d_B), d_B >= 1e-5 + EPS: at most 1.19 EPS w_B / d_B.  Either way
    |z32 - z64| <= 3 EPS max(w / d) over the two bins, plus the interpolation's own roundings.  -> (mask, bound)"""
    cdf, k = det["cdf"], det["k"]
    kl, kr = torch.clamp(k - 1, min=0), torch.clamp(k + 1, max=cdf.shape[-1] - 1)
    ck, bk = torch.gather(cdf, 1, k), torch.gather(det["bins"], 1, k)
    bound, clear = torch.zeros_like(det["gap"]), torch.ones_like(det["gap"], dtype=torch.bool)
    for kn in (kl, kr):
        dn = (torch.gather(cdf, 1, kn) - ck).abs()
        width = (torch.gather(det["bins"], 1, kn) - bk).abs()
        here = kn != k
        clear &= ~here | (dn >= 1e-5 + EPS)
        bound = torch.maximum(bound, torch.where(here, width * (3 * EPS) / dn.clamp(min=1e-5), torch.zeros_like(dn)))
    big = torch.maximum(det["lo"].abs(), det["hi"].abs())
    return (det["gap"] < EPS) & clear & ((det["denom_raw"] - 1e-5).abs() >= EPS), bound + 8 * ulp32(big)[:, None]


def fine_bound(det):
    """|z32 - z64| allowed for a well-conditioned draw: a CDF error of EPS on either end of the bin, divided by the bin's probability
    mass, times the bin's width; plus the interpolation's own roundings (8 float32 ulp of the largest bin)"""
    big = torch.maximum(det["lo"].abs(), det["hi"].abs())
    return (det["bins_a"] - det["bins_b"]).abs() * (2 * EPS) / det["denom"] + 8 * ulp32(big)[:, None]


def check_fine(z32, det):
    """the rule of both inverse-CDF kernels against float64 -> (share of ill-conditioned draws, worst error / bound of the others).  An
    ill-conditioned draw need only lie inside the row's [min(bins), max(bins)]; a draw near a step between two sound bins (near_step) is
    held to its own bound and does not count as ill-conditioned.  Rows whose float64 chain is not finite or whose CDF does not ascend
    (negative weights: searchsorted has no defined answer) must be left out by the caller."""
    z32 = f64(z32)
    step, step_bound = near_step(det)
    ill = ill_conditioned(det) & ~step
    assert bool(((z32 >= det["lo"][:, None]) & (z32 <= det["hi"][:, None]))[ill].all()), "an ill-conditioned draw left [min(bins), max(bins)]"
    ratio = (z32 - det["z"]).abs() / torch.where(step, step_bound, fine_bound(det))
    ratio = float(ratio[~ill].max()) if bool((~ill).any()) else 0.0
    share = float(ill.double().mean()) if ill.numel() else 0.0
    return share, ratio


def usable_rows(det, weights):
    """rows the fine-sample rule applies to: a finite float64 chain over a proper pdf (weights >= 0, so the CDF ascends and searchsorted
    has a defined answer).  A ray whose box lies behind it has descending samples, negative 'weights' and exponentials that overflow
    float32 long before float64: the merge invariants cover it, no value rule does."""
    fin = torch.isfinite(det["z"]).all(-1) & torch.isfinite(det["cdf"]).all(-1) & torch.isfinite(det["bins"]).all(-1)
    return fin & (f64(weights) >= 0).all(-1)


def composites(sigma, rgbc, z, nears, fars, num_steps, soft, thr, detach_bg=False, detach_mask=False, dtype=D, variants=(0, 1, 2)):
    """the three weights_sum_i calls of run() (renderer.py:384-402) on per-ray tensors sigma [N, S], rgbc [N, S, 4] -> out_ray [3, N, 6]
    (image rgb, depth, weights_sum, render_mask of all / fg / bg), differentiable in sigma and rgbc.  dtype float32 = the float32 oracle.
    variants: the composites to build; the rows of the others are zeros that no graph hangs on."""
    N, S = sigma.shape
    z, nears, fars = (torch.as_tensor(a).detach().cpu().to(dtype) for a in (z, nears, fars))
    nears, fars = nears.reshape(N, 1), fars.reshape(N, 1)
    sd = (fars - nears) / num_steps
    if S == 1:
        # weights_sum_i builds its last delta from a slice that is empty for a single sample.  One sample is that sample followed, sample_dist
        # further on, by one of zero density: its delta is sample_dist, the added sample weighs nothing and nothing behind a sample acts on it
        sigma = torch.cat([sigma, torch.zeros_like(sigma)], 1)
        rgbc = torch.cat([rgbc, torch.zeros_like(rgbc)], 1)
        z = torch.cat([z, z + sd], 1)
    rgb, conf = rgbc[..., :3], rgbc[..., 3:4]
    thr = float(np.float32(thr))                                       # the kernel receives the threshold as a float
    e = torch.sigmoid((conf - thr) * 100) if soft else (conf > 0.5).to(dtype)
    kw = dict(train_conf=True, detach_bg=detach_bg, detach_mask_from_field=detach_mask)
    s = sigma[..., None]
    call = [lambda: to.weights_sum_i(sd, s, z, nears, fars, rgb, (1, N), conf, is_all=True, **kw),
            lambda: to.weights_sum_i(sd, s * e, z, nears, fars, rgb, (1, N), conf, if_fg=True, **kw),
            lambda: to.weights_sum_i(sd, s * (1 - e), z, nears, fars, rgb, (1, N), conf, **kw)]
    out = []
    for v in range(3):
        if v not in variants:
            out.append(torch.zeros(N, 6, dtype=dtype))
            continue
        r = call[v]()
        out.append(torch.cat([r['image'].reshape(N, 3), r['depth'].reshape(N, 1), r['weights_sum'].reshape(N, 1), r['render_mask'].reshape(N, 1)], -1))
    return torch.stack(out)


def composites_with_grads(sigma, rgbc, z, nears, fars, num_steps, soft, thr, g_out, detach_bg=False, detach_mask=False, dtype=D):
    """-> out_ray [3, N, 6], d sum(out_ray * g_out) / d sigma [N, S], / d rgbc [N, S, 4].  A variant whose g_out is all zero is computed
    (its output is compared) but kept out of the loss: autograd would carry its zero seed through as 0 * NaN on a ray that misses the box,
    where the kernel — and the reference's own loss, which never touches such a variant — adds nothing."""
    s = torch.as_tensor(sigma).detach().cpu().to(dtype).requires_grad_(True)
    c = torch.as_tensor(rgbc).detach().cpu().to(dtype).requires_grad_(True)
    g = torch.as_tensor(g_out).detach().cpu().to(dtype)
    used = tuple(v for v in range(3) if bool((g[v] != 0).any()))
    with torch.no_grad():
        out = composites(s, c, z, nears, fars, num_steps, soft, thr, detach_bg, detach_mask, dtype)
    loss = (s * 0).sum() + (c * 0).sum() + (composites(s, c, z, nears, fars, num_steps, soft, thr, detach_bg, detach_mask, dtype, used) * g).sum()
    loss.backward()
    return out, s.grad, c.grad


def recon_loss(out_ray, rgb_gt, mask_gt, w_rgb, w_conf):
    """utils_init_nerf.py:220-234 on out_ray [3, N, 6] -> loss, d loss / d out_ray"""
    o = f64(out_ray).requires_grad_(True)
    loss = w_rgb * ((o[0, :, 0:3] - f64(rgb_gt).reshape(-1, 3)) ** 2).mean()
    if mask_gt is not None:
        loss = loss + w_conf * ((o[0, :, 5] - f64(mask_gt).reshape(-1)) ** 2).mean()
    loss.backward()
    return loss.detach(), o.grad


def run(field, rays_o, rays_d, nears, fars, aabb, num_steps, upsample_steps, training=True, soft_mask=True, conf_thr=0.5, detach_bg=False,
        detach_mask=False, draws=None):
    """renderer.py:278-405 in float64 from float32 rays, nears / fars and draws -> dict(z_vals, out_ray [3, N, 6], weights [N, S])"""
    draws = draws or {}
    o, d, aabb = f64(rays_o).reshape(-1, 3), f64(rays_d).reshape(-1, 3), f64(aabb)
    N = o.shape[0]
    z, xyz = sample_coarse(o, d, nears, fars, aabb, num_steps, draws.get('z'))
    sig_c = field.density(xyz.reshape(-1, 3))['sigma'].view(N, num_steps)
    w, mid = coarse_weights(z, sig_c, nears, fars, num_steps)
    nz = to.sample_pdf(mid, w[:, 1:-1], upsample_steps, det=not training, u=f64(draws.get('u')) if training else None)
    z_all = torch.sort(torch.cat([z, nz], dim=1), dim=1).values
    xyz_all = points(o, d, z_all, aabb)
    S = z_all.shape[1]
    sigma, rgbc, _ = field(xyz_all.reshape(-1, 3), d[:, None].expand(N, S, 3).reshape(-1, 3))
    out = composites(sigma.view(N, S), rgbc.view(N, S, 4), z_all, nears, fars, num_steps, soft_mask, conf_thr, detach_bg, detach_mask)
    sd = ((f64(fars) - f64(nears)) / num_steps).reshape(N, 1)
    weights = to.weights_sum_i(sd, sigma.view(N, S, 1), z_all, f64(nears).reshape(N, 1), f64(fars).reshape(N, 1), rgbc.view(N, S, 4)[..., :3], (1, N),
                               rgbc.view(N, S, 4)[..., 3:4], is_all=True)['weights']
    return dict(z_vals=z_all, out_ray=out, weights=weights)
