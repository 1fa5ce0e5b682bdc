"""CPU: the float64 restatement of the run() kernels (tests/run_restatement.py) against the reference's own outputs under tests/golden/, and
what tests/test_gpu_run_shapes.py assumes about its inputs (tests/run_testlib.py): every ray class comes out of near_far_from_aabb as built,
and the ill-conditioned inverse-CDF draws of every configuration stay under the 2 % cap."""
import numpy as np
import pytest
import torch

import run_restatement as rr
import run_testlib as tl
from oracle import c_oracle as co
from oracle import torch_oracle as to
from oracle.toy_field import ToyField


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_sample_pdf_float64_against_reference_golden(golden):
    """the tolerances of test_sample_pdf_kernel_against_reference_golden: the golden outputs are float32, so a draw within rounding of a
    CDF step may sit in the neighbouring bin there"""
    g = golden("sample_pdf")
    det = rr.sample_pdf_detail(g["bins"], g["weights"], 16, det=True)
    assert torch.equal(det["z"], to.sample_pdf(rr.f64(g["bins"]), rr.f64(g["weights"]), 16, det=True))       # one definition
    err = np.abs(det["z"].numpy() - g["out_det"])
    assert err.max() < 2e-5 and (err > 2e-6).mean() < 0.02, (float(err.max()), float((err > 2e-6).mean()))
    rnd = rr.sample_pdf_detail(g["bins"], g["weights"], 16, det=False, u=g["u"])
    assert torch.equal(rnd["z"], to.sample_pdf(rr.f64(g["bins"]), rr.f64(g["weights"]), 16, det=False, u=rr.f64(g["u"])))
    err = np.abs(rnd["z"].numpy() - g["out_rnd"])
    assert (err > 2e-6).mean() < 0.01, float((err > 2e-6).mean())
    # and the reference's float32 outputs pass the rule the kernels are held to
    for d, out in ((det, g["out_det"]), (rnd, g["out_rnd"])):
        share, ratio = rr.check_fine(out, d)
        assert share <= 0.02 and ratio <= 1.0, (share, ratio)
    # the float32 det draw of the oracle is what it was
    assert to.sample_pdf(T(g["bins"]), T(g["weights"]), 16, det=True).dtype == torch.float32


def test_weights_sum_i_float64_against_reference_golden(golden):
    """the tolerances of test_weights_sum_i_method_against_reference_golden"""
    g = golden("weights_sum_i")
    N = g["sigmas"].shape[0]
    for tag, kw in (("plain", {}), ("detach", dict(detach_bg=True, detach_mask_from_field=True))):
        s, c = rr.f64(g["sigmas"]).requires_grad_(True), rr.f64(g["rgbs"]).requires_grad_(True)
        res = to.weights_sum_i(rr.f64(g["sample_dist"]), s, rr.f64(g["z"]), rr.f64(g["nears"]), rr.f64(g["fars"]), c, (1, N), rr.f64(g["masks"]),
                               is_all=True, **kw)
        assert res["image"].dtype == torch.float64
        loss = (res['image'] ** 2).sum() + res['weights_sum'].sum() + (res['render_mask'] * 0.3).sum() + res['depth'].sum()
        loss.backward()
        for k in ("image", "depth", "render_mask", "weights_sum", "weights"):
            np.testing.assert_allclose(res[k].detach().numpy(), g[f"{tag}__{k}"], rtol=1e-5, atol=2e-6, err_msg=f"{tag}:{k}")
        gs, gc = g[f"{tag}__grad_sigmas"], g[f"{tag}__grad_rgbs"]
        np.testing.assert_allclose(s.grad.numpy(), gs, rtol=2e-4, atol=2e-5 * float(np.abs(gs).max()), err_msg=tag + ":grad_sigmas")
        np.testing.assert_allclose(c.grad.numpy(), gc, rtol=2e-4, atol=2e-6, err_msg=tag + ":grad_rgbs")
    # the composites helper is those calls: its first variant is the golden 'plain' call (k: the fixture's sample_dist as a step count)
    k = float(((g["fars"] - g["nears"]) / g["sample_dist"]).mean())
    out = rr.composites(rr.f64(g["sigmas"])[..., 0], torch.cat([rr.f64(g["rgbs"]), rr.f64(g["masks"])], -1), g["z"], g["nears"], g["fars"], k, True, 0.5)
    np.testing.assert_allclose(out[0, :, 0:3].numpy(), g["plain__image"].reshape(N, 3), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(out[0, :, 4].numpy(), g["plain__weights_sum"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(out[0, :, 5].numpy(), g["plain__render_mask"].reshape(N), rtol=1e-5, atol=2e-6)


RUN_CASES = {
    "train_T8": dict(training=True, perturb=True, kw=dict(num_steps=8, upsample_steps=8)),
    "train_T64": dict(training=True, perturb=True, kw=dict(num_steps=64, upsample_steps=64)),
    "eval_T64": dict(training=False, perturb=False, kw=dict(num_steps=64, upsample_steps=64)),
    "train_T16_hardmask": dict(training=True, perturb=True, kw=dict(num_steps=16, upsample_steps=16, soft_mask=False)),
    "train_T16_detach": dict(training=True, perturb=True, kw=dict(num_steps=16, upsample_steps=16, detach_bg=True, detach_mask=True)),
}


@pytest.mark.parametrize("tag", list(RUN_CASES))
def test_run_float64_against_reference_golden(golden, tag):
    """the 1e-4 of test_run_matches_reference_golden (the golden run is float32; its hard-mask and inverse-CDF decisions are its own)"""
    g = golden("run")
    c = RUN_CASES[tag]
    st = int(g[f"{tag}__stride"])
    o, d = g["rays_o"][0, ::st], g["rays_d"][0, ::st]
    aabb = np.array([-2.0, -2, -2, 2, 2, 2], np.float32)
    nears, fars = co.near_far_from_aabb(o, d, aabb, 0.01)
    draws = {k: g[f"{tag}__{k}"] for k in ("z", "u") if c["perturb"] and f"{tag}__{k}" in g}
    res = rr.run(ToyField(), o, d, nears, fars, aabb, training=c["training"], draws=draws, **c["kw"])
    N = o.shape[0]
    out = res["out_ray"].numpy()
    for v, sub in enumerate(("", "fg_", "bg_")):
        np.testing.assert_allclose(out[v, :, 0:3], g[f"{tag}__{sub}image"].reshape(N, 3), rtol=0, atol=1e-4, err_msg=sub + "image")
        np.testing.assert_allclose(out[v, :, 3], g[f"{tag}__{sub}depth"].reshape(N), rtol=0, atol=1e-4, err_msg=sub + "depth")
        np.testing.assert_allclose(out[v, :, 4], g[f"{tag}__{sub}weights_sum"].reshape(N), rtol=0, atol=1e-4, err_msg=sub + "weights_sum")
        np.testing.assert_allclose(out[v, :, 5], g[f"{tag}__{sub}render_mask"].reshape(N), rtol=0, atol=1e-4, err_msg=sub + "render_mask")
    np.testing.assert_allclose(res["weights"].numpy(), g[f"{tag}__weights"], rtol=0, atol=1e-4)


@pytest.mark.parametrize("bound", tl.BOUNDS)
def test_every_ray_class_comes_out_as_built(bound):
    for n_per in (11, 167):
        o, d, cls = tl.make_rays(bound, n_per, seed=int(bound * 10))
        nears, fars = co.near_far_from_aabb(o.numpy(), d.numpy(), tl.aabb_of(bound).numpy(), tl.MIN_NEAR)
        tl.assert_ray_classes(cls, nears, fars)


def _merge_detail(case, z, nears, fars, sigma, u):
    """the float64 chain behind the fine samples of one merge configuration (rows: all rays) and the rows the rule of (b) applies to"""
    T, t, N, det = case[:4]
    w, mid = rr.coarse_weights(z, sigma, nears, fars, T)
    with np.errstate(all="ignore"):
        d = rr.sample_pdf_detail(mid, w[:, 1:-1], t, det=det, u=u)
    return d, rr.usable_rows(d, w) & torch.isfinite(rr.f64(z)).all(-1)


def test_ill_conditioned_draws_of_the_merge_configurations_stay_under_the_cap():
    """(b) of test_gpu_run_shapes: with the coarse samples as the float32 oracle forms them (the kernel's differ by an ulp), every
    configuration has at most 2 % ill-conditioned draws among the rays the rule applies to — and the float32 oracle's own fine samples pass
    the rule.  As it stands: 1506 rows under the rule, worst share of a configuration 0.41 %, float32 oracle at most 0.37 of the bound."""
    worst, worst_ratio, rows = 0.0, 0.0, 0
    for case in tl.merge_cases():
        T_, t, N, det, bound = case[:5]
        o, d, cls, noise, sigma, u = tl.merge_inputs(case)
        aabb = tl.aabb_of(bound)
        nears, fars = co.near_far_from_aabb(o.numpy(), d.numpy(), aabb.numpy(), tl.MIN_NEAR)
        z = tl.coarse_f32(o, d, T(nears), T(fars), aabb, T_, noise)
        det64, ok = _merge_detail(case, z, nears, fars, sigma, u)
        if not bool(ok.any()):
            continue
        rows += int(ok.sum())
        sub = {k: v[ok] for k, v in det64.items()}
        # the float32 oracle's fine samples of the same rows
        zz, nn, ff, ss = z[ok], T(nears)[ok][:, None], T(fars)[ok][:, None], sigma[ok]
        deltas = torch.cat([zz[:, 1:] - zz[:, :-1], (ff - nn) / T_], -1)
        al = 1 - torch.exp(-deltas * ss)
        w32 = al * torch.cumprod(torch.cat([torch.ones_like(al[:, :1]), 1 - al + 1e-15], -1), -1)[:, :-1]
        nz32 = to.sample_pdf(zz[:, :-1] + 0.5 * deltas[:, :-1], w32[:, 1:-1], t, det=det, u=None if det else u[ok])
        share, ratio = rr.check_fine(nz32, sub)
        worst, worst_ratio = max(worst, share), max(worst_ratio, ratio)
        assert share <= 0.02, (case, share)
        assert ratio <= 1.0, (case, ratio)
    print(f"merge configurations: {rows} rows under the rule, worst ill-conditioned share {worst:.4f}, float32 oracle worst error / bound {worst_ratio:.3f}")
    assert rows > 1000


def test_ill_conditioned_draws_of_the_sample_pdf_configurations_stay_under_the_cap():
    """(c) of test_gpu_run_shapes, same statement for cnerf_sample_pdf's configurations"""
    worst, worst_ratio = 0.0, 0.0
    for nb in tl.PDF_BINS:
        for ns in tl.PDF_SAMPLES:
            for B in tl.PDF_B:
                for kind in ("zero", "spike"):
                    bins, w = tl.pdf_inputs(nb, B, kind)
                    for det in (True, False):
                        u = None if det else tl.pdf_u(B, ns)
                        d = rr.sample_pdf_detail(bins, w, ns, det=det, u=u)
                        share, ratio = rr.check_fine(to.sample_pdf(bins, w, ns, det=det, u=u), d)
                        worst, worst_ratio = max(worst, share), max(worst_ratio, ratio)
                        assert share <= 0.02 and ratio <= 1.0, (nb, ns, B, kind, det, share, ratio)
    print(f"sample_pdf configurations: worst ill-conditioned share {worst:.4f}, float32 oracle worst error / bound {worst_ratio:.3f}")


def test_composite_and_loss_restatements_are_the_float32_oracle_in_float64():
    """composites(dtype=float32) is the oracle the existing kernel tests use; in float64 it differs from it by float32 rounding only, gradients
    included; recon_loss is F.mse_loss's formulation"""
    import torch.nn.functional as F
    sig, rgbc, z, nears, fars = tl.composite_inputs(5, 65, first=0)
    g = torch.randn(3, 5, 6, generator=torch.Generator().manual_seed(1))
    fin = [0, 1, 2, 3]                                                     # (row 4 is the missed ray: NaN depth on both sides)
    for soft in (True, False):
        o64, gs64, gc64 = rr.composites_with_grads(sig, rgbc, z, nears, fars, 32, soft, 0.5, g)
        o32, gs32, gc32 = rr.composites_with_grads(sig, rgbc, z, nears, fars, 32, soft, 0.5, g, dtype=torch.float32)
        assert o64.dtype == torch.float64 and o32.dtype == torch.float32
        assert torch.equal(torch.isnan(o64), torch.isnan(o32)) and bool(torch.isnan(o64[:, 4, 3]).all()) and not bool(torch.isnan(o64[:, fin]).any())
        np.testing.assert_allclose(o32[:, fin].numpy(), o64[:, fin].numpy(), rtol=0, atol=2e-6)
        np.testing.assert_allclose(gs32[fin].numpy(), gs64[fin].numpy(), rtol=1e-3, atol=1e-5 * max(1.0, float(gs64[fin].abs().max())))
    out = torch.rand(3, 300, 6, generator=torch.Generator().manual_seed(2))
    rgb, mask = torch.rand(300, 3), (torch.rand(300) > 0.5).float()
    loss, grad = rr.recon_loss(out, rgb, mask, 1.0, 0.3)
    o = out.double().requires_grad_(True)
    ref = F.mse_loss(o[0, :, 0:3], rgb.double()) + 0.3 * F.mse_loss(o[0, :, 5], mask.double())
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) < 1e-12 and torch.allclose(grad, o.grad, atol=1e-15)
