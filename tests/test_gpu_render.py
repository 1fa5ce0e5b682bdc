"""GPU parity of the renderer-level path: ray generation, Adam, NeRFRenderer.run with the closed-form field against the
reference's golden vectors, the real field (grid + MLPs) against the oracle field, run()/run_cuda() end to end incl.
gradients.  Tolerance for rendered rgb/depth/weights: 1e-4 absolute in fp32 (north_star)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import c_oracle as co          # noqa: E402
from oracle import torch_oracle as to      # noqa: E402
from oracle.toy_field import ToyField      # noqa: E402


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_generate_rays_against_reference_golden(golden):
    from customnerf_amd.nerf.provider_utils import generate_rays, get_rays
    g = golden("rays")
    for tag in ("32", "64", "24x40"):
        fx, fy, cx, cy, H, W = g[f"get_rays_{tag}__intr"]
        H, W = int(H), int(W)
        pose = torch.eye(4).unsqueeze(0).clone()
        pose[0, :3, :4] = T(g[f"get_rays_{tag}__c2w"])
        r = get_rays(pose.cuda(), (fx, fy, cx, cy), H, W)
        np.testing.assert_allclose(r['rays_d'].cpu().numpy(), g[f"get_rays_{tag}__d"], rtol=0, atol=1e-6)
        np.testing.assert_array_equal(r['rays_o'].cpu().numpy(), g[f"get_rays_{tag}__o"])
        c2w = T(g[f"gen_rays_{tag}__c2w"])[None].cuda()
        for level in (1, 2):
            o, d = generate_rays(c2w, fx, fy, cx, cy, H, W, level, 'nerfstudio')
            np.testing.assert_array_equal(o[0].cpu().numpy(), g[f"gen_rays_{tag}_l{level}__o"])
            np.testing.assert_allclose(d[0].cpu().numpy(), g[f"gen_rays_{tag}_l{level}__d"], rtol=0, atol=1e-6)


def test_fisheye_rays_against_reference_golden(golden):
    """OPENCV_FISHEYE branch of _generate_rays (provider.py:421-433): k_generate_rays convention 2 against directions the reference's own
    radial_and_tangential_undistort produced (tests/golden/make_golden.py section 7b), and against the oracle restatement."""
    from customnerf_amd.nerf.provider_utils import generate_rays
    g = golden("rays_fisheye")
    for tag in ("24x40", "32"):
        fx, fy, cx, cy, H, W, level = g[f"{tag}__intr"]
        H, W = int(H), int(W)
        c2w = T(g[f"{tag}__c2w"])[None]
        dist = [float(v) for v in g[f"{tag}__dist"]]
        o, d = generate_rays(c2w.cuda(), fx, fy, cx, cy, H, W, level, 'nerfstudio', distortion=dist)
        np.testing.assert_array_equal(o[0].cpu().numpy(), g[f"{tag}__o"])
        # ten Newton steps + sin / cos of the device's libm vs glibc: a few float32 ulps on unit vectors
        np.testing.assert_allclose(d[0].cpu().numpy(), g[f"{tag}__d"], rtol=0, atol=2e-6)
        o_ref, d_ref = to.generate_rays_fisheye(c2w, fx, fy, cx, cy, H, W, level, dist)
        np.testing.assert_allclose(d[0].cpu().numpy(), d_ref[0].numpy(), rtol=0, atol=2e-6)
    # zero distortion: the un-distortion is the identity, only the theta mapping remains (|coord| -> angle from the optical axis)
    o, d = generate_rays(T(g["32__c2w"])[None].cuda(), 20.0, 20.0, 16.3, 15.8, 32, 32, 1.0, 'nerfstudio', distortion=[0.0] * 6)
    assert torch.isfinite(d).all() and torch.allclose(d.norm(dim=-1), torch.ones(1, 32, 32, device='cuda'), atol=1e-5)


def test_fisheye_scene_loader(tmp_path):
    """NerfstudioScene on an OPENCV_FISHEYE transforms.json: the distortion parameters reach the ray kernel (the loader used to raise)."""
    import json
    from customnerf_amd.nerf.provider import NerfstudioScene
    from customnerf_amd.nerf.provider_utils import generate_rays
    frames = []
    rng = np.random.default_rng(0)
    for i in range(4):
        m = np.eye(4)
        a = 2 * np.pi * i / 4
        m[:3, 3] = [2 * np.cos(a), 0.3, 2 * np.sin(a)]
        frames.append({"file_path": f"images/{i:03d}.png", "transform_matrix": m.tolist()})
    meta = dict(camera_model="OPENCV_FISHEYE", fl_x=30.0, fl_y=30.0, cx=16.0, cy=12.0, w=32, h=24, k1=0.05, k2=-0.01, k3=0.002, k4=0.0, frames=frames)
    (tmp_path / "transforms.json").write_text(json.dumps(meta))
    sc = NerfstudioScene(str(tmp_path), load_images=False)
    assert sc.distortion == [0.05, -0.01, 0.002, 0.0, 0.0, 0.0]
    o, d = generate_rays(sc.camera_to_world.cuda(), 30.0, 30.0, 16.0, 12.0, 24, 32, 1.0, 'nerfstudio', distortion=sc.distortion)
    assert torch.equal(sc.rays_d.view(-1, 3), d.view(-1, 3))
    o2, d2 = generate_rays(sc.camera_to_world.cuda(), 30.0, 30.0, 16.0, 12.0, 24, 32, 1.0, 'nerfstudio')
    assert not torch.allclose(d, d2, atol=1e-3)                     # and they differ from the pinhole rays


def test_sample_pdf_kernel_against_reference_golden(golden):
    """renderer.sample_pdf (k_sample_pdf) against outputs of the reference's own sample_pdf (renderer.py:21-55)."""
    from customnerf_amd.nerf.renderer import sample_pdf
    g = golden("sample_pdf")
    bins, w = cuda(g["bins"]), cuda(g["weights"])
    out = sample_pdf(bins, w, 16, det=True)
    # the CDF is a wave scan here and a sequential cumsum there: a handful of samples differ by a few float32 ulps of values around 1..3
    err = np.abs(out.cpu().numpy() - g["out_det"])
    assert err.max() < 2e-5 and (err > 2e-6).mean() < 0.02, (float(err.max()), float((err > 2e-6).mean()))
    out = sample_pdf(bins, w, 16, det=False, u=cuda(g["u"]))
    ref = g["out_rnd"]
    err = np.abs(out.cpu().numpy() - ref)
    # the CDF is a wave scan here and a sequential cumsum there: a draw that lands within float rounding of a CDF step may pick the neighbouring bin
    assert (err > 2e-6).mean() < 0.01, float((err > 2e-6).mean())
    # a ragged n_samples (not a multiple of the wave) and the wave-strided bins loop
    gen = torch.Generator().manual_seed(3)
    bins = torch.sort(torch.rand(37, 130, generator=gen), dim=-1).values
    w = torch.rand(37, 129, generator=gen)
    u = torch.rand(37, 75, generator=gen)
    ref = to.sample_pdf(bins, w, 75, det=False, u=u)
    out = sample_pdf(bins.cuda(), w.cuda(), 75, det=False, u=u.cuda())
    err = (out.cpu() - ref).abs()
    assert float((err > 2e-6).float().mean()) < 0.01
    with pytest.raises(RuntimeError):
        sample_pdf(bins, w, 8, det=True)                             # CPU tensors: there is no CPU path


def test_weights_sum_i_method_against_reference_golden(golden):
    """NeRFRenderer.weights_sum_i (the compositing kernel behind the reference's signature) against outputs and gradients of the reference's
    own weights_sum_i (renderer.py:407-474), plain and with detach_bg / detach_mask_from_field."""
    g = golden("weights_sum_i")
    N = g["sigmas"].shape[0]
    for tag, kw in (("plain", {}), ("detach", dict(detach_bg=True, detach_mask_from_field=True))):
        model = _toy_renderer(**kw)
        s, c = cuda(g["sigmas"]).requires_grad_(True), cuda(g["rgbs"]).requires_grad_(True)
        res = model.weights_sum_i(cuda(g["sample_dist"]), s, None, None, None, cuda(g["z"]), cuda(g["nears"]), cuda(g["fars"]), c, (1, N),
                                  masks=cuda(g["masks"]), is_all=True)
        loss = (res['image'] ** 2).sum() + res['weights_sum'].sum() + (res['render_mask'] * 0.3).sum() + res['depth'].sum()
        loss.backward()
        for k in ("image", "depth", "render_mask", "weights_sum", "weights"):
            np.testing.assert_allclose(res[k].detach().cpu().numpy(), g[f"{tag}__{k}"], rtol=1e-5, atol=2e-6, err_msg=f"{tag}:{k}")
        np.testing.assert_array_equal(res["mask"].cpu().numpy(), g[f"{tag}__mask"])
        gs, gc = g[f"{tag}__grad_sigmas"], g[f"{tag}__grad_rgbs"]
        np.testing.assert_allclose(s.grad.cpu().numpy(), gs, rtol=2e-4, atol=2e-5 * float(np.abs(gs).max()), err_msg=tag + ":grad_sigmas")
        np.testing.assert_allclose(c.grad.cpu().numpy(), gc, rtol=2e-4, atol=2e-6, err_msg=tag + ":grad_rgbs")


def test_run_without_train_conf_and_unsupported_counts():
    """the reference's run() leaves its result dict empty without opt.train_conf (renderer.py:383-405); sample counts outside the kernels'
    range are rejected loudly (there is no torch slow path behind run())"""
    model = _toy_renderer(train_conf=0)
    o = torch.zeros(1, 4, 3, device='cuda'); o[..., 2] = 3.0
    d = torch.zeros(1, 4, 3, device='cuda'); d[..., 2] = -1.0
    assert model.run(o, d, num_steps=8, upsample_steps=8) == {}
    model = _toy_renderer()
    with pytest.raises(ValueError):
        model.run(o, d, num_steps=8, upsample_steps=0)
    with pytest.raises(ValueError):
        model.run(o, d, num_steps=256, upsample_steps=8)
    with pytest.raises(RuntimeError):
        model.run(o.cpu(), d.cpu(), num_steps=8, upsample_steps=8)


def test_adam_step_matches_torch():
    from customnerf_amd.optim import adam_step
    torch.manual_seed(0)
    n = 100003
    p = torch.randn(n).cuda(); g = torch.randn(n).cuda() * 1e-3
    ref_p = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref_p], lr=5e-3, betas=(0.9, 0.99), eps=1e-15)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ph = torch.empty(n, dtype=torch.half).cuda()
    for step in range(1, 6):
        gi = g * step
        ref_p.grad = gi.clone()
        opt.step()
        gbuf = (gi * 128.0).clone()                       # as if produced under a 128x loss scale
        adam_step(p, gbuf, m, v, lr=5e-3, betas=(0.9, 0.99), eps=1e-15, step=step, grad_scale_inv=1 / 128.0, zero_grad=True, p_half=ph)
        assert torch.all(gbuf == 0)
    np.testing.assert_allclose(p.cpu().numpy(), ref_p.detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert torch.equal(ph, p.half())


CASES = {
    "train_T8": dict(training=True, kw=dict(num_steps=8, upsample_steps=8, perturb=True), opt={}),
    "train_T64": dict(training=True, kw=dict(num_steps=64, upsample_steps=64, perturb=True), opt={}),
    "eval_T64": dict(training=False, kw=dict(num_steps=64, upsample_steps=64, perturb=False), opt={}),
    "train_T16_hardmask": dict(training=True, kw=dict(num_steps=16, upsample_steps=16, perturb=True), opt=dict(soft_mask=False)),
    "train_T16_detach": dict(training=True, kw=dict(num_steps=16, upsample_steps=16, perturb=True), opt=dict(detach_bg=True, detach_mask_from_field=True)),
}


def _toy_renderer(**opt_kw):
    from customnerf_amd.nerf.renderer import NeRFRenderer
    from customnerf_amd.scene import make_opt

    class ToyRenderer(NeRFRenderer):
        def __init__(self, opt):
            super().__init__(opt)
            self.f = ToyField()

        def forward(self, x, d, *a, **k):
            return self.f(x, d)

        def density(self, x):
            return self.f.density(x)
    return ToyRenderer(make_opt(**opt_kw)).cuda()


@pytest.mark.parametrize("tag", list(CASES))
def test_run_matches_reference_golden(golden, tag):
    """NeRFRenderer.run on the GPU (HIP near_far + renderer logic) replaying the reference's own RNG draws."""
    g = golden("run")
    c = CASES[tag]
    st = int(g[f"{tag}__stride"])
    rays_o, rays_d = T(g["rays_o"])[:, ::st].contiguous().cuda(), T(g["rays_d"])[:, ::st].contiguous().cuda()
    draws = {"light": T(g[f"{tag}__light"])}
    if f"{tag}__z" in g:
        draws["z"] = T(g[f"{tag}__z"])
    if f"{tag}__u" in g:
        draws["u"] = T(g[f"{tag}__u"])
    model = _toy_renderer(**c["opt"])
    model.train(c["training"])
    res = model.run(rays_o, rays_d, _draws=draws, **c["kw"])
    for k in ("image", "depth", "render_mask", "weights_sum", "weights"):
        np.testing.assert_allclose(res[k].cpu().numpy(), g[f"{tag}__{k}"], rtol=0, atol=1e-4, err_msg=f"{tag}:{k}")
    np.testing.assert_array_equal(res["mask"].cpu().numpy(), g[f"{tag}__mask"])
    for sub in ("fg", "bg"):
        for k in ("image", "depth", "render_mask", "weights_sum"):
            np.testing.assert_allclose(res[sub][k].cpu().numpy(), g[f"{tag}__{sub}_{k}"], rtol=0, atol=1e-4, err_msg=f"{tag}:{sub}.{k}")


def _fields(seed=0, **kw):
    """A NeRFNetwork (product, GPU) and a FieldRef (oracle, CPU) with identical parameters, cfg1-like geometry."""
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.scene import make_opt
    from customnerf_amd import tcnn
    tcnn.set_default_dtype(torch.float32)
    geo = dict(num_levels=4, log2_hashmap_size=19, desired_resolution=2048, n_hidden_geo=1)
    geo.update(kw)
    opt = make_opt(cuda_ray=geo.pop("cuda_ray", False), **geo)
    model = NeRFNetwork(opt).cuda()
    ref = to.FieldRef(bound=opt.bound, num_levels=opt.num_levels, level_dim=2, base_resolution=16, log2_hashmap_size=opt.log2_hashmap_size,
                      desired_resolution=opt.desired_resolution, gridtype='hash', n_hidden_geo=opt.n_hidden_geo, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        ref.pos_en.embeddings.copy_((torch.rand(ref.pos_en.embeddings.shape, generator=g) * 2 - 1) * 0.5)   # U(-.5,.5): visible features
        model.pos_en.embeddings.copy_(ref.pos_en.embeddings.cuda())
        model.network.params.copy_(ref.network.cuda())
        model.density_network.params.copy_(ref.density_network.cuda())
        model.rgb_network.params.copy_(ref.rgb_network.cuda())
    return model, ref, opt


def test_field_forward_backward_vs_oracle():
    model, ref, opt = _fields()
    rng = np.random.default_rng(0)
    P = 3000
    x = ((rng.random((P, 3)) * 2 - 1) * 1.9).astype(np.float32)
    d = rng.standard_normal((P, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    s_ref, c_ref, _ = ref(T(x), T(d))
    s, c, _ = model(cuda(x), cuda(d))
    np.testing.assert_allclose(s.detach().cpu().numpy(), s_ref.detach().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(c.detach().cpu().numpy(), c_ref.detach().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(model.density(cuda(x))['sigma'].detach().cpu().numpy(), s_ref.detach().numpy(), rtol=1e-4, atol=1e-5)
    gs = rng.standard_normal(P).astype(np.float32) * 0.1
    gc = rng.standard_normal((P, 4)).astype(np.float32)
    torch.autograd.backward([s_ref, c_ref], [T(gs), T(gc)])
    torch.autograd.backward([s, c], [cuda(gs), cuda(gc)])
    for name, a, b in (("grid", model.pos_en.embeddings.grad, ref.pos_en.embeddings.grad), ("net", model.network.params.grad, ref.network.grad),
                       ("den", model.density_network.params.grad, ref.density_network.grad), ("rgb", model.rgb_network.params.grad, ref.rgb_network.grad)):
        b = b.numpy()
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=1e-3, atol=1e-4 * max(1.0, float(np.abs(b).max())), err_msg=name)


def test_run_end_to_end_vs_oracle_cfg1():
    """cfg1 (32x32 view, L=4 grid, one-hidden-layer MLPs): full run() forward + loss + backward vs the CPU oracle."""
    from customnerf_amd import scene as sc
    model, ref, opt = _fields()
    model.train()
    H = W = 32
    pose = torch.eye(4).unsqueeze(0).clone()
    pose[0, :3, :4] = T(sc.camera_pose(1, opencv=True))
    o, d = to.get_rays(pose, sc.intrinsics(H, W), H, W)
    g = torch.Generator().manual_seed(5)
    draws = dict(light=torch.randn(3, generator=g), z=torch.rand(H * W, 16, generator=g), u=torch.rand(H * W, 16, generator=g))
    kw = dict(num_steps=16, upsample_steps=16, perturb=True)
    r_ref = to.run(ref, o, d, torch.tensor([-2.0, -2, -2, 2, 2, 2]), opt.min_near, training=True, draws=draws, **kw)
    r = model.run(o.cuda(), d.cuda(), _draws=draws, **kw)
    for k in ("image", "depth", "render_mask", "weights_sum", "weights"):
        np.testing.assert_allclose(r[k].detach().cpu().numpy(), r_ref[k].detach().numpy(), rtol=0, atol=1e-4, err_msg=k)
    # fg/bg split the density with sigmoid((conf - thr) * 100) (renderer.py:387): the x100 gain amplifies fp32 rounding
    # differences of the confidence channel (different matmul summation order GPU vs CPU) by two orders of
    # magnitude, so these two composites are compared at 1e-3; the unsplit image above holds 1e-4.
    for sub in ("fg", "bg"):
        for k in ("image", "depth", "weights_sum"):
            np.testing.assert_allclose(r[sub][k].detach().cpu().numpy(), r_ref[sub][k].detach().numpy(), rtol=0, atol=1e-3, err_msg=sub + k)
    rgb_gt, m_gt = sc.targets(1, H, W, seed=3)

    def loss_of(res, dev):
        return ((res['image'].reshape(-1, 3) - rgb_gt[0].to(dev)) ** 2).mean() + 0.01 * ((res['render_mask'].reshape(-1) - m_gt[0].reshape(-1).to(dev)) ** 2).mean()
    l_ref, l = loss_of(r_ref, 'cpu'), loss_of(r, 'cuda')
    assert abs(l.item() - l_ref.item()) < 1e-5
    l_ref.backward(); l.backward()
    for name, a, b in (("grid", model.pos_en.embeddings.grad, ref.pos_en.embeddings.grad), ("net", model.network.params.grad, ref.network.grad),
                       ("den", model.density_network.params.grad, ref.density_network.grad), ("rgb", model.rgb_network.params.grad, ref.rgb_network.grad)):
        b = b.numpy()
        # the wave scans (transmittance products, CDF sums) associate differently from torch's sequential cumprod / cumsum: rounding-level
        # differences that survive the cancellation in the smallest weight-gradient elements (5e-7 absolute floor)
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=2e-3, atol=5e-4 * max(1e-3, float(np.abs(b).max())), err_msg=name)


def test_run_cuda_train_and_eval_vs_oracle():
    from customnerf_amd import scene as sc
    model, ref, opt = _fields(cuda_ray=True)
    grid = sc.sphere_density_grid(2, 128, 2.0, 1.0, 100.0)
    bitfield = co.packbits(grid, 10.0)
    model.density_grid.copy_(cuda(grid))
    model.density_bitfield.copy_(cuda(bitfield))
    H = W = 32
    pose = torch.eye(4).unsqueeze(0).clone()
    pose[0, :3, :4] = T(sc.camera_pose(6, opencv=True))
    o, d = to.get_rays(pose, sc.intrinsics(H, W), H, W)
    aabb = torch.tensor([-2.0, -2, -2, 2, 2, 2])
    noises = torch.rand(H * W, generator=torch.Generator().manual_seed(9))
    # --- training branch
    model.train()
    r_ref = to.run_cuda_train(ref, o, d, aabb, 2.0, bitfield, 2, 128, noises.numpy(), 0, 1024, 1e-4)
    r = model.run_cuda(o.cuda(), d.cuda(), perturb=True, force_all_rays=True, _noises=noises.cuda())
    np.testing.assert_array_equal(r['rays'].cpu().numpy(), r_ref['rays'])          # compacted ray indices: bit-exact
    assert model.step_counter[0].cpu().numpy().tolist() == r_ref['counter'].tolist()
    for k in ("image", "depth", "weights_sum"):
        np.testing.assert_allclose(r[k].detach().cpu().numpy().reshape(r_ref[k].shape), r_ref[k].detach().numpy(), rtol=0, atol=1e-4, err_msg=k)
    np.testing.assert_array_equal(r['mask'].cpu().numpy().reshape(-1), r_ref['mask'].numpy())
    l_ref = (r_ref['image'] ** 2).sum() + r_ref['weights_sum'].sum()
    l = (r['image'] ** 2).sum() + r['weights_sum'].sum()
    l_ref.backward(); l.backward()
    for name, a, b in (("grid", model.pos_en.embeddings.grad, ref.pos_en.embeddings.grad), ("net", model.network.params.grad, ref.network.grad),
                       ("den", model.density_network.params.grad, ref.density_network.grad), ("rgb", model.rgb_network.params.grad, ref.rgb_network.grad)):
        b = b.numpy()
        # the wave scans (transmittance products, CDF sums) associate differently from torch's sequential cumprod / cumsum: rounding-level
        # differences that survive the cancellation in the smallest weight-gradient elements (5e-7 absolute floor)
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=2e-3, atol=5e-4 * max(1e-3, float(np.abs(b).max())), err_msg=name)
    # --- inference branch
    model.eval()
    with torch.no_grad():
        e = model.run_cuda(o.cuda(), d.cuda(), perturb=False, T_thresh=1e-4)
    e_ref = to.run_cuda_eval(ref, o, d, aabb, 2.0, bitfield, 2, 128, 0, 1024, 1e-4)
    for k in ("image", "depth", "weights_sum"):
        np.testing.assert_allclose(e[k].cpu().numpy().reshape(e_ref[k].shape), e_ref[k], rtol=0, atol=1e-4, err_msg="eval " + k)
    # training and inference composites agree with each other too (same samples, same field)
    np.testing.assert_allclose(e['image'].cpu().numpy().reshape(-1, 3), r_ref['image'].detach().numpy(), rtol=0, atol=5e-3)


def test_update_extra_state_builds_occupancy():
    """update_extra_state (renderer.py:1658-1715): morton3D + density query + EMA + packbits on the device."""
    model, ref, opt = _fields(cuda_ray=True)
    torch.manual_seed(0)
    model.update_extra_state()
    dg = model.density_grid.cpu().numpy()
    assert dg.min() >= 0 and model.mean_density > 0
    np.testing.assert_allclose(model.mean_density, float(dg.astype(np.float64).mean()), rtol=1e-6)
    thr = min(model.mean_density, model.density_thresh)
    np.testing.assert_array_equal(model.density_bitfield.cpu().numpy(), co.packbits(dg, thr))
    # the gaussian blob (network_grid.py:150-156) makes the centre dense: the centre cell must be occupied in cascade 0
    centre = co.morton3D(np.array([[64, 64, 64]], np.int32))[0]
    assert dg[0, centre] > thr


def test_update_extra_state_kernels_vs_oracle():
    """The occupancy refresh kernels (csrc/occupancy.hip) against the restatement of renderer.py:1658-1715 with the same jitter draws: two
    refreshes on a 32^3 grid (the second one exercises the 0.95 decay against the first one's densities), with a cell marked invalid (< 0)."""
    model, ref, opt = _fields(cuda_ray=True)
    Hs = 32
    model.grid_size = Hs
    model.density_grid = torch.zeros(model.cascade, Hs ** 3, device='cuda')
    model.density_bitfield = torch.zeros(model.cascade * Hs ** 3 // 8, dtype=torch.uint8, device='cuda')
    model.density_grid[1, 77] = -1.0                                  # an invalid cell stays untouched and out of the mean
    grid_ref = model.density_grid.cpu().numpy()
    gen = torch.Generator().manual_seed(4)
    for it in range(2):
        rand = [torch.rand(Hs ** 3, 3, generator=gen) for _ in range(model.cascade)]
        model.local_step = 0
        model.update_extra_state(_rand=rand)
        grid_ref, mean_ref, bits_ref = to.update_extra_state(ref, grid_ref, opt.bound, model.cascade, Hs, 0.95, opt.density_thresh, rand)
        dg = model.density_grid.cpu().numpy()
        assert dg[1, 77] == -1.0
        np.testing.assert_allclose(dg, grid_ref, rtol=2e-4, atol=1e-5)
        np.testing.assert_allclose(model.mean_density, mean_ref, rtol=1e-4)
        bits = model.density_bitfield.cpu().numpy()
        assert np.unpackbits(bits ^ bits_ref).sum() <= 4              # cells within rounding of the threshold may differ
        np.testing.assert_array_equal(bits, co.packbits(dg, min(model.mean_density, model.density_thresh)))
    assert model.iter_density == 2


def test_update_extra_state_matches_reference_golden(golden):
    """NeRFRenderer.update_extra_state (occupancy kernels) replaying the jitter draws of the reference's own loop (renderer.py:1658-1715 run on a
    16^3 grid with the toy density, tests/golden/occupancy.npz): density grid, mean density, bitfield and the sample-count ring, two refreshes."""
    g = golden("occupancy")
    H, cas = int(g["grid_size"]), int(g["cascade"])
    model = _toy_renderer(cuda_ray=True, bound=float(g["bound"]), density_thresh=float(g["density_thresh"]))
    assert model.cascade == cas
    model.grid_size = H
    model.density_grid = T(g["grid0"]).cuda().contiguous()
    model.density_bitfield = torch.zeros(cas * H ** 3 // 8, dtype=torch.uint8, device="cuda")
    for rnd in range(2):
        model.local_step = 3 + rnd
        model.step_counter[:4, 0] = torch.tensor([100, 200, 301, 77], dtype=torch.int32, device="cuda")
        model.update_extra_state(decay=float(g["decay"]), S=H, _rand=[T(r) for r in g[f"r{rnd}__rand"]])
        want = g[f"r{rnd}__grid"]
        dg = model.density_grid.cpu().numpy()
        assert np.array_equal(dg < 0, want < 0) and np.array_equal(dg[want < 0], want[want < 0])
        np.testing.assert_allclose(dg, want, rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(float(model.mean_density), float(g[f"r{rnd}__mean_density"]), rtol=1e-6)
        thr = min(float(g[f"r{rnd}__mean_density"]), float(g["density_thresh"]))
        diff = np.unpackbits(model.density_bitfield.cpu().numpy() ^ g[f"r{rnd}__bitfield"], bitorder="little").astype(bool)
        assert not diff[np.abs(want.reshape(-1) - thr) > 1e-4].any() and diff.sum() <= 2
        assert model.mean_count == int(g[f"r{rnd}__mean_count"]) and model.local_step == 0


def _rand_composite_inputs(N=200, S=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    sig = (torch.rand(N, S, generator=g) * 6) ** 2
    rgbc = torch.rand(N, S, 4, generator=g)
    z = torch.sort(torch.rand(N, S, generator=g) * 3 + 0.3, dim=-1).values
    nears, fars = z[:, 0] - 0.05, z[:, -1] + 0.2
    return sig, rgbc, z, nears, fars


@pytest.mark.parametrize("soft,dbg,dmask", [(True, False, False), (False, False, False), (True, True, True)])
def test_composite_run_kernel_vs_oracle(soft, dbg, dmask):
    """cnerf_composite_run fwd + bwd against weights_sum_i x3 of the oracle (which is pinned to the reference's golden vectors)."""
    from customnerf_amd.nerf.render_ops import composite_run
    N, S, T = 200, 128, 64
    sig, rgbc, z, nears, fars = _rand_composite_inputs(N, S)
    s_ref, c_ref = sig.clone().requires_grad_(True), rgbc.clone().requires_grad_(True)
    rgb, conf = c_ref[..., :3], c_ref[..., 3:4]
    sd = ((fars - nears) / T)[:, None]
    e = torch.sigmoid((conf - 0.5) * 100) if soft else (conf > 0.5).float()
    kw = dict(train_conf=True, detach_bg=dbg, detach_mask_from_field=dmask)
    refs = [to.weights_sum_i(sd, s_ref[..., None], z, nears[:, None], fars[:, None], rgb, (1, N), conf, is_all=True, **kw),
            to.weights_sum_i(sd, s_ref[..., None] * e, z, nears[:, None], fars[:, None], rgb, (1, N), conf, if_fg=True, **kw),
            to.weights_sum_i(sd, s_ref[..., None] * (1 - e), z, nears[:, None], fars[:, None], rgb, (1, N), conf, **kw)]
    s, c = sig.clone().cuda().requires_grad_(True), rgbc.clone().cuda().requires_grad_(True)
    out_ray, out_w = composite_run(s, c, z.cuda(), nears.cuda(), fars.cuda(), T, soft, 0.5, dbg, dmask)
    g = torch.Generator().manual_seed(3)
    loss_ref, loss = 0, 0
    for v, r in enumerate(refs):
        o = out_ray[v].detach().cpu().numpy()
        np.testing.assert_allclose(o[:, 0:3], r['image'].detach().numpy().reshape(N, 3), rtol=0, atol=2e-6)
        np.testing.assert_allclose(o[:, 3], r['depth'].detach().numpy().reshape(N), rtol=0, atol=2e-6)
        np.testing.assert_allclose(o[:, 4], r['weights_sum'].detach().numpy(), rtol=0, atol=2e-6)
        np.testing.assert_allclose(o[:, 5], r['render_mask'].detach().numpy().reshape(N), rtol=0, atol=2e-6)
        np.testing.assert_allclose(out_w[v].cpu().numpy(), r['weights'].detach().numpy(), rtol=0, atol=1e-6)
        gi = torch.randn(N, 6, generator=g)
        loss_ref = loss_ref + (r['image'].reshape(N, 3) * gi[:, :3]).sum() + (r['depth'].reshape(N) * gi[:, 3]).sum() + \
            (r['weights_sum'] * gi[:, 4]).sum() + (r['render_mask'].reshape(N) * gi[:, 5]).sum()
        loss = loss + (out_ray[v] * gi.cuda()).sum()
    loss_ref.backward(); loss.backward()
    gs_ref, gc_ref = s_ref.grad.numpy(), c_ref.grad.numpy()
    np.testing.assert_allclose(s.grad.cpu().numpy(), gs_ref, rtol=1e-3, atol=1e-5 * max(1.0, float(np.abs(gs_ref).max())))
    np.testing.assert_allclose(c.grad.cpu().numpy(), gc_ref, rtol=1e-3, atol=1e-5 * max(1.0, float(np.abs(gc_ref).max())))


@pytest.mark.parametrize("used,S,T", [((1,), 128, 64), ((0, 2), 100, 50), ((2,), 40, 20), ((0, 1, 2), 200, 100), ((), 128, 64)])
def test_composite_backward_with_unused_variants_and_chunk_counts(used, S, T):
    """the compositing backward skips a variant none of whose outputs received a gradient (round 6) and keeps a ray's samples in registers for
    1 .. 4 chunks of 64: gradients into any subset of the three variants, for 40 / 100 / 128 / 200 samples per ray, against autograd on the oracle"""
    from customnerf_amd.nerf.render_ops import composite_run
    N = 150
    sig, rgbc, z, nears, fars = _rand_composite_inputs(N, S, seed=S)
    s_ref, c_ref = sig.clone().requires_grad_(True), rgbc.clone().requires_grad_(True)
    rgb, conf = c_ref[..., :3], c_ref[..., 3:4]
    sd = ((fars - nears) / T)[:, None]
    e = torch.sigmoid((conf - 0.5) * 100)
    kw = dict(train_conf=True, detach_bg=False, detach_mask_from_field=False)
    refs = [to.weights_sum_i(sd, s_ref[..., None], z, nears[:, None], fars[:, None], rgb, (1, N), conf, is_all=True, **kw),
            to.weights_sum_i(sd, s_ref[..., None] * e, z, nears[:, None], fars[:, None], rgb, (1, N), conf, if_fg=True, **kw),
            to.weights_sum_i(sd, s_ref[..., None] * (1 - e), z, nears[:, None], fars[:, None], rgb, (1, N), conf, **kw)]
    s, c = sig.clone().cuda().requires_grad_(True), rgbc.clone().cuda().requires_grad_(True)
    out_ray, _ = composite_run(s, c, z.cuda(), nears.cuda(), fars.cuda(), T, True, 0.5, False, False)
    g = torch.Generator().manual_seed(5)
    loss_ref, loss = (s_ref * 0).sum() + (c_ref * 0).sum(), (out_ray * 0).sum()
    for v in used:
        r = refs[v]
        gi = torch.randn(N, 6, generator=g)
        loss_ref = loss_ref + (r['image'].reshape(N, 3) * gi[:, :3]).sum() + (r['depth'].reshape(N) * gi[:, 3]).sum() + \
            (r['weights_sum'] * gi[:, 4]).sum() + (r['render_mask'].reshape(N) * gi[:, 5]).sum()
        loss = loss + (out_ray[v] * gi.cuda()).sum()
    loss_ref.backward(); loss.backward()
    gs_ref, gc_ref = s_ref.grad.numpy(), c_ref.grad.numpy()
    np.testing.assert_allclose(s.grad.cpu().numpy(), gs_ref, rtol=1e-3, atol=1e-5 * max(1.0, float(np.abs(gs_ref).max())))
    np.testing.assert_allclose(c.grad.cpu().numpy(), gc_ref, rtol=1e-3, atol=1e-5 * max(1.0, float(np.abs(gc_ref).max())))
    if not used:
        assert float(s.grad.abs().max()) == 0.0 and float(c.grad.abs().max()) == 0.0


def test_composite_forward_computes_the_requested_variants_only():
    """cnerf_composite_run_indexed_variants: with the mask of the reconstruction trainer (first composite only) the first composite and its
    gradients are the bits of the three-composite launch, the other rows are zeros; run(fg_bg=False) drops the 'fg' / 'bg' entries"""
    from customnerf_amd.nerf import render_ops
    N, S, T = 300, 128, 64
    sig, rgbc, z, nears, fars = _rand_composite_inputs(N, S, seed=9)
    z, nears, fars = z.cuda(), nears.cuda(), fars.cuda()
    ident = torch.arange(N * S, dtype=torch.int32, device='cuda').view(N, S)
    g = torch.randn(N, 6, generator=torch.Generator().manual_seed(4)).cuda()
    outs = []
    for variants in (7, 1, 5):
        s_, c_ = sig.reshape(-1).clone().cuda().requires_grad_(True), rgbc.reshape(-1, 4).clone().cuda().requires_grad_(True)
        o = render_ops.composite_run_indexed(s_, c_, z, ident, nears, fars, T, True, 0.5, variants=variants)
        (o[0] * g).sum().backward()
        outs.append((o.detach(), s_.grad, c_.grad))
    full, first, first_bg = outs
    assert torch.equal(full[0][0], first[0][0]) and torch.equal(full[1], first[1]) and torch.equal(full[2], first[2])
    assert float(first[0][1:].abs().max()) == 0.0
    assert torch.equal(full[0][0], first_bg[0][0]) and torch.equal(full[0][2], first_bg[0][2]) and float(first_bg[0][1].abs().max()) == 0.0
    assert float(full[0][1].abs().max()) > 0.0


def test_sampling_kernels_vs_oracle():
    """cnerf_sample_coarse / cnerf_sample_fine_merge against the torch restatement of renderer.py:310-363 (train and det)."""
    from customnerf_amd.nerf import render_ops
    from customnerf_amd import scene as sc
    H = W = 24
    pose = torch.eye(4).unsqueeze(0).clone()
    pose[0, :3, :4] = T(sc.camera_pose(3, opencv=True))
    o, d = to.get_rays(pose, sc.intrinsics(H, W), H, W)
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    N = o.shape[0]
    aabb = torch.tensor([-2.0, -2, -2, 2, 2, 2])
    nears, fars = co.near_far_from_aabb(o.numpy(), d.numpy(), aabb.numpy(), 0.01)
    nears, fars = T(nears), T(fars)
    for Tn, tn, train in ((64, 64, True), (16, 48, True), (64, 64, False), (100, 7, True)):
        g = torch.Generator().manual_seed(Tn)
        zr, u = torch.rand(N, Tn, generator=g), torch.rand(N, tn, generator=g)
        sigma = (torch.rand(N, Tn, generator=g) * 5) ** 2
        sigma[::7] = 0                                               # all-zero weights rows -> the denom < 1e-5 branch
        # oracle (same formulas as to.run)
        z = nears[:, None] + (fars - nears)[:, None] * torch.linspace(0.0, 1.0, Tn)[None]
        sd = ((fars - nears) / Tn)[:, None]
        z = z + (zr - 0.5) * sd
        xyz = torch.min(torch.max(o[:, None] + d[:, None] * z[..., None], aabb[:3]), aabb[3:])
        deltas = torch.cat([z[:, 1:] - z[:, :-1], sd], dim=-1)
        alphas = 1 - torch.exp(-deltas * sigma)
        w = alphas * torch.cumprod(torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-15], dim=-1), dim=-1)[:, :-1]
        mid = z[:, :-1] + 0.5 * deltas[:, :-1]
        nz = to.sample_pdf(mid, w[:, 1:-1], tn, det=not train, u=u if train else None)
        z_all_ref = torch.sort(torch.cat([z, nz], dim=1), dim=1).values
        xyz_all_ref = torch.min(torch.max(o[:, None] + d[:, None] * z_all_ref[..., None], aabb[:3]), aabb[3:])
        # kernels
        zc, xc = render_ops.sample_coarse(o.cuda(), d.cuda(), nears.cuda(), fars.cuda(), aabb.cuda(), Tn, zr.cuda())
        np.testing.assert_allclose(zc.cpu().numpy(), z.numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(xc.cpu().numpy(), xyz.numpy(), rtol=0, atol=2e-6)
        za, xa = render_ops.sample_fine_merge(o.cuda(), d.cuda(), nears.cuda(), fars.cuda(), aabb.cuda(), zc, sigma.cuda(), tn, u.cuda() if train else None)
        za_np = za.cpu().numpy()
        assert np.all(np.diff(za_np, axis=1) >= 0)                   # sorted
        # sample_pdf has a discontinuity (`denom < 1e-5 -> 1`, renderer.py:51) and a searchsorted: when a cdf gap sits within float
        # rounding of 1e-5 the two sides (wave scan here, sequential cumsum in the oracle) can legitimately take different
        # branches.  Everything else must agree to 2e-5; the ill-conditioned draws must stay rare and inside one coarse bin.
        dz = np.abs(za_np - z_all_ref.numpy())
        assert (dz > 2e-5).mean() < 5e-3, (dz > 2e-5).mean()
        assert dz.max() < float((fars - nears).max()) / Tn
        dx = np.abs(xa.cpu().numpy() - xyz_all_ref.numpy())
        assert (dx > 5e-5).mean() < 5e-3


@pytest.mark.parametrize("tag", ["train_T64", "eval_T64", "train_T16_hardmask", "train_T16_detach"])
def test_fused_run_matches_reference_golden(golden, tag):
    """The fused run() (sampling + composite kernels) with the closed-form field, replaying the reference's RNG draws."""
    from customnerf_amd.nerf.renderer import NeRFRenderer
    from customnerf_amd.scene import make_opt
    g = golden("run")
    c = CASES[tag]
    st = int(g[f"{tag}__stride"])
    rays_o, rays_d = T(g["rays_o"])[:, ::st].contiguous().cuda(), T(g["rays_d"])[:, ::st].contiguous().cuda()
    draws = {"light": T(g[f"{tag}__light"])}
    if f"{tag}__z" in g:
        draws["z"] = T(g[f"{tag}__z"])
    if f"{tag}__u" in g:
        draws["u"] = T(g[f"{tag}__u"])

    class ToyFused(NeRFRenderer):
        supports_dir_group = True

        def __init__(self, opt):
            super().__init__(opt)
            self.f = ToyField()

        def forward(self, x, d, *a, dir_group=1, **k):
            dd = d.reshape(-1, 3).repeat_interleave(dir_group, dim=0)
            return self.f(x, dd)

        def density(self, x):
            return self.f.density(x)
    model = ToyFused(make_opt(**c["opt"])).cuda()
    model.train(c["training"])
    res = model.run(rays_o, rays_d, _draws=draws, **c["kw"])
    assert 'z_vals' in res                                          # the fused path ran
    for k in ("image", "depth", "render_mask", "weights_sum", "weights"):
        np.testing.assert_allclose(res[k].cpu().numpy(), g[f"{tag}__{k}"], rtol=0, atol=1e-4, err_msg=f"{tag}:{k}")
    np.testing.assert_array_equal(res["mask"].cpu().numpy(), g[f"{tag}__mask"])
    for sub in ("fg", "bg"):
        for k in ("image", "depth", "render_mask", "weights_sum"):
            np.testing.assert_allclose(res[sub][k].cpu().numpy(), g[f"{tag}__{sub}_{k}"], rtol=0, atol=1e-4, err_msg=f"{tag}:{sub}.{k}")


@pytest.mark.parametrize("fp16", [False, True], ids=["f32", "f16"])
def test_split_evaluation_equals_merged_evaluation(fp16):
    """run() with the coarse samples' grid features gathered once (split sample list + src_index compositing) against the
    reference's order (sorted merged list, coarse samples encoded twice): same outputs bit for bit (the field is evaluated
    per sample, the compositing kernels do the same operations in the same order), same gradients up to summation order."""
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider_utils import generate_rays
    tcnn.set_default_dtype(torch.float16 if fp16 else torch.float32)
    try:
        torch.manual_seed(0)
        opt = sc.make_opt(fp16=fp16, num_levels=16)
        model = NeRFNetwork(opt).cuda().train()
        with torch.no_grad():
            model.pos_en.embeddings.uniform_(-0.5, 0.5)
        H = W = 24
        o, d = generate_rays(torch.from_numpy(sc.poses(1)).cuda(), *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
        o, d = o.view(1, H * W, 3), d.view(1, H * W, 3)
        g = torch.Generator().manual_seed(5)
        draws = dict(z=torch.rand(H * W, 32, generator=g), u=torch.rand(H * W, 32, generator=g))
        rgb_gt, m_gt = sc.targets(1, H, W, seed=3)
        res, grads = {}, {}
        # True = split sample list, block-wise field evaluation; "plain" = split list with the separate density pass and one full evaluation;
        # False = the reference's merged order
        for mode in (True, "plain", False):
            opt.split_eval = bool(mode)
            opt.blockwise_field = mode != "plain"
            model.zero_grad(set_to_none=True)
            with torch.autocast('cuda', dtype=torch.float16, enabled=fp16):
                r = model.run(o, d, num_steps=32, upsample_steps=32, perturb=True, _draws=draws)
            loss = ((r['image'].reshape(-1, 3) - rgb_gt[0].cuda()) ** 2).mean() + 0.1 * ((r['render_mask'].reshape(-1) - m_gt[0].reshape(-1).cuda()) ** 2).mean() \
                + 0.1 * r['fg']['image'].mean() + 0.1 * r['bg']['depth'].mean()
            loss.backward()
            res[mode] = r
            grads[mode] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        for other in ("plain", False):
            for k in ("image", "depth", "render_mask", "weights_sum", "weights", "sigma", "rgbs", "edit_mask", "z_vals"):
                assert torch.equal(res[True][k], res[other][k]), (other, k)
            for sub in ("fg", "bg"):
                for k in ("image", "depth", "render_mask", "weights_sum", "weights"):
                    assert torch.equal(res[True][sub][k], res[other][sub][k]), (other, sub, k)
            assert set(grads[True]) == set(grads[other]) and "pos_en.embeddings" in grads[True]
            for n in grads[True]:
                a, b = grads[True][n].float(), grads[other][n].float()
                scale = float(b.abs().max())
                assert scale > 0, n
                assert float((a - b).abs().max()) <= (2e-3 if fp16 else 1e-5) * scale, (other, n, float((a - b).abs().max()), scale)
    finally:
        tcnn.set_default_dtype(torch.float16)


def test_strided_gather_and_indexed_composite_reduce_to_the_plain_forms():
    from customnerf_amd.gridencoder import GridEncoder
    from customnerf_amd.nerf import render_ops
    torch.manual_seed(1)
    enc = GridEncoder(input_dim=3, num_levels=8, level_dim=2, base_resolution=16, log2_hashmap_size=15, desired_resolution=512).cuda()
    with torch.no_grad():
        enc.embeddings.uniform_(-1, 1)
    x = torch.rand(3000, 3, device="cuda")
    xs = x * 2 - 1
    full = enc.encode(xs, bound=1, half=False)                         # [L, 3000, 2]
    unit = (xs + 1) / 2                                                # the [0,1] coordinates encode() derives (grid.py:156), bit for bit
    buf = torch.full((8, 3000 + 77, 2), -7.0, device="cuda")
    enc.encode_into(unit[:1000], buf, 0, half=False)
    enc.encode_into(unit[1000:], buf, 1000, half=False)
    assert torch.equal(buf[:, :3000], full) and bool((buf[:, 3000:] == -7.0).all())      # rows outside the gathers are untouched
    # indexed composite with the identity index == plain composite; with a per-ray permutation == plain composite of the permuted inputs
    N, S = 150, 96
    g = torch.Generator(device="cuda").manual_seed(3)
    sig = torch.rand(N * S, device="cuda", generator=g) * 5
    rgbc = torch.rand(N * S, 4, device="cuda", generator=g)
    z = torch.sort(torch.rand(N, S, device="cuda", generator=g) * 3 + 0.5, dim=1)[0]
    nears, fars = torch.full((N,), 0.5, device="cuda"), torch.full((N,), 3.5, device="cuda")
    ident = torch.arange(N * S, device="cuda", dtype=torch.int32).view(N, S)
    plain = render_ops.composite_run(sig.view(N, S), rgbc.view(N, S, 4), z, nears, fars, 48, True, 0.5)
    idx_ray = render_ops.composite_run_indexed(sig, rgbc, z, ident, nears, fars, 48, True, 0.5)
    idx_w, idx_sig, idx_rgbc = render_ops.composite_run_indexed_aux(sig, rgbc, z, ident, nears, fars, 48, True, 0.5)      # the lazy by-products
    assert torch.equal(plain[0], idx_ray) and torch.equal(plain[1], idx_w)
    assert torch.equal(idx_sig.view(-1), sig) and torch.equal(idx_rgbc.view(-1, 4), rgbc)
    perm = torch.stack([torch.randperm(S, device="cuda", generator=g) for _ in range(N)]).to(torch.int32) + (torch.arange(N, device="cuda", dtype=torch.int32) * S)[:, None]
    sig_p, rgbc_p = sig[perm.long().view(-1)], rgbc[perm.long().view(-1)]
    sig_l, rgbc_l = sig.clone().requires_grad_(True), rgbc.clone().requires_grad_(True)
    sig_m, rgbc_m = sig_p.clone().requires_grad_(True), rgbc_p.clone().requires_grad_(True)
    a = render_ops.composite_run_indexed(sig_l, rgbc_l, z, perm.contiguous(), nears, fars, 48, True, 0.5)
    b = render_ops.composite_run(sig_m.view(N, S), rgbc_m.view(N, S, 4), z, nears, fars, 48, True, 0.5)
    assert torch.equal(a, b[0])
    w = torch.rand(3, N, 6, device="cuda", generator=g)
    (a * w).sum().backward(); (b[0] * w).sum().backward()
    assert torch.equal(sig_l.grad[perm.long().view(-1)], sig_m.grad) and torch.equal(rgbc_l.grad[perm.long().view(-1)], rgbc_m.grad)


def test_samplers_write_the_grid_coordinates_bit_for_bit():
    """cnerf_sample_coarse_unit / cnerf_sample_fine_merge_split_unit: the [0,1] grid coordinates they emit equal torch's
    (xyz + bound) / (2 bound) on the positions they emit (gridencoder/grid.py:156), for a power-of-two and a non-power-of-two bound."""
    from customnerf_amd.nerf import render_ops
    g = torch.Generator(device="cuda").manual_seed(5)
    N, T, t = 777, 48, 40
    for bound in (2.0, 1.3):
        o = (torch.rand(N, 3, device="cuda", generator=g) - 0.5) * bound
        d = torch.nn.functional.normalize(torch.randn(N, 3, device="cuda", generator=g), dim=-1)
        aabb = torch.tensor([-bound] * 3 + [bound] * 3, device="cuda")
        nears, fars = torch.full((N,), 0.05, device="cuda"), torch.full((N,), 2.5 * bound, device="cuda")
        noise, u = torch.rand(N, T, device="cuda", generator=g), torch.rand(N, t, device="cuda", generator=g)
        unit_c = torch.empty(N, T, 3, device="cuda")
        z, xyz = render_ops.sample_coarse(o, d, nears, fars, aabb, T, noise, unit_out=unit_c, bound=bound)
        z_ref, xyz_ref = render_ops.sample_coarse(o, d, nears, fars, aabb, T, noise)
        assert torch.equal(z, z_ref) and torch.equal(xyz, xyz_ref)
        assert torch.equal(unit_c, (xyz + bound) / (2 * bound))
        sig = torch.rand(N, T, device="cuda", generator=g) * 3
        unit_f = torch.empty(N, t, 3, device="cuda")
        za, xf, src = render_ops.sample_fine_merge_split(o, d, nears, fars, aabb, z, sig, t, u, unit_fine_out=unit_f, bound=bound)
        zb, xg, srb = render_ops.sample_fine_merge_split(o, d, nears, fars, aabb, z, sig, t, u)
        assert torch.equal(za, zb) and torch.equal(xf, xg) and torch.equal(src, srb)
        assert torch.equal(unit_f, (xf + bound) / (2 * bound))


@pytest.mark.parametrize("half", [False, True])
def test_field_matches_reference_glue_golden(golden, half):
    """The fused field (k_grid_fwd / k_field_fwd / k_field_bwd_* / the binned scatter) at the reference field's own geometry (tiledgrid, T = 2^21,
    desired 8192: network_grid.py:89-96) against tests/golden/field.npz — the reference's own NeRFNetwork glue over this build's restatements of
    the kernel and of tinycudann: outputs and every parameter gradient (float32), and within float16 rounding under autocast."""
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.scene import make_opt
    from customnerf_amd import tcnn
    g = golden("field")
    tcnn.set_default_dtype(torch.float16 if half else torch.float32)
    try:
        opt = make_opt(fp16=half, grid_type='tiledgrid', log2_hashmap_size=21, desired_resolution=8192)
        model = NeRFNetwork(opt).cuda()
        n = int(g["n_embeddings"])
        assert model.pos_en.embeddings.shape[0] == n
        idx = torch.arange(n, dtype=torch.float64)
        with torch.no_grad():
            model.pos_en.embeddings.copy_(torch.stack([torch.sin(idx * 0.37) * 0.5, torch.cos(idx * 0.11 + 1.3) * 0.5], -1).float().cuda())
            model.pos_en.invalidate_half_table()
            model.network.params.copy_(T(g["network__params"]).cuda())
            model.density_network.params.copy_(T(g["density_network__params"]).cuda())
            model.rgb_network.params.copy_(T(g["rgb_network__params"]).cuda())
        x, d = T(g["x"]).cuda(), T(g["d"]).cuda()
        with torch.autocast('cuda', dtype=torch.float16, enabled=half):
            sigma, rad, _ = model(x, d)
            dens = model.density(x)["sigma"]
            loss = (sigma.float() * T(g["w_sigma"]).cuda() * 0.01).sum() + (rad.float() * T(g["w_rad"]).cuda()).sum()
        loss.backward()
        rt, at = (2e-2, 2e-3) if half else (2e-4, 1e-6)
        np.testing.assert_allclose(sigma.float().detach().cpu().numpy(), g["sigma"], rtol=rt, atol=at)
        np.testing.assert_allclose(dens.float().detach().cpu().numpy(), g["density_sigma"], rtol=rt, atol=at)
        np.testing.assert_allclose(rad.float().detach().cpu().numpy(), g["radiances"], rtol=rt, atol=at)
        for nm in ("network", "density_network", "rgb_network"):
            got, want = getattr(model, nm).params.grad.float().cpu().numpy(), g[f"{nm}__grad"]
            assert np.abs(got - want).max() <= (3e-2 if half else 5e-4) * np.abs(want).max(), nm
        ge = model.pos_en.embeddings.grad.float().cpu()
        want = torch.zeros_like(ge)
        want[torch.from_numpy(g["grad_emb_idx"])] = T(g["grad_emb_val"])
        assert float((ge - want).abs().max()) <= (3e-2 if half else 5e-4) * float(want.abs().max())
        if not half:
            assert np.array_equal(torch.nonzero(ge.abs().sum(-1)).reshape(-1).numpy(), g["grad_emb_idx"])
    finally:
        tcnn.set_default_dtype(torch.float32)


def test_coarse_sampler_with_the_slab_test_folded_in():
    """cnerf_sample_coarse_unit_aabb (near_far_from_aabb + stratified samples + grid coordinates in one launch) against the two separate
    launches: the same bits, rays that miss the box included"""
    from customnerf_amd import raymarching
    from customnerf_amd.nerf import render_ops
    g = torch.Generator(device="cuda").manual_seed(4)
    N, T = 3000, 64
    o = (torch.rand(N, 3, device="cuda", generator=g) * 2 - 1) * 3.5
    d = torch.nn.functional.normalize(torch.randn(N, 3, device="cuda", generator=g), dim=-1)
    d[:7, 0] = 0.0                                                       # axis-parallel components: 1 / 0 in the slab test
    aabb = torch.tensor([-2.0, -2, -2, 2, 2, 2], device="cuda")
    noise = torch.rand(N, T, device="cuda", generator=g)
    nears, fars = raymarching.near_far_from_aabb(o, d, aabb, 0.01)
    xyz_a, unit_a = torch.empty(N, T, 3, device="cuda"), torch.empty(N, T, 3, device="cuda")
    z_a, _ = render_ops.sample_coarse(o, d, nears, fars, aabb, T, noise, xyz_out=xyz_a, unit_out=unit_a, bound=2.0)
    xyz_b, unit_b = torch.empty(N, T, 3, device="cuda"), torch.empty(N, T, 3, device="cuda")
    n_b, f_b, z_b, _ = render_ops.sample_coarse_aabb(o, d, aabb, 0.01, T, noise, xyz_b, unit_b, 2.0)
    assert torch.equal(n_b, nears) and torch.equal(f_b, fars)
    same = lambda a, b: torch.equal(a, b) or torch.equal(torch.nan_to_num(a, nan=1e30), torch.nan_to_num(b, nan=1e30))
    assert same(z_a, z_b) and same(xyz_a, xyz_b) and same(unit_a, unit_b)
    assert int((nears > 1e30).sum()) > 0                                 # the case has rays that miss the box


# ---- run() + loss + backward at the HEADLINE configuration (cfg2: 128x128 view, 64 + 64 samples, L16 two-hidden-layer field)
# f16 bounds: measured on MI355X (printed by the test), pinned at 3x; f32: the 1e-4 of north_star
_HEADLINE_F16_PIN = {            # geometry -> {quantity: 3 x measured max abs error (image / depth / weights_sum) or max|diff| / max|ref| (gradients)}
    # measured (round 6, MI355X): image 2.25e-5, depth 3.9e-6, weights_sum 1.25e-6, grid 2.69e-2, net 7.62e-2, den 6.29e-2, rgb 5.67e-3
    "hash_T19": dict(image=7e-5, depth=1.2e-5, weights_sum=4e-6, grid=8.1e-2, net=0.23, den=0.19, rgb=1.7e-2),
    # measured: image 4.55e-5, depth 2.28e-5, weights_sum 1.85e-6, grid 4.78e-2, net 3.20e-2, den 1.18e-1, rgb 1.34e-2
    "bear_tiled_T21": dict(image=1.4e-4, depth=7e-5, weights_sum=6e-6, grid=0.145, net=0.1, den=0.36, rgb=4.1e-2),
    # 24 levels (the two-launch field backward).  measured: image 3.91e-5, depth 3.46e-6, weights_sum 1.19e-6, grid 7.42e-2, net 5.20e-2,
    # den 1.06e-1 (3x would exceed the loose bound: den stays at _HEADLINE_F16_LOOSE), rgb 8.09e-3
    "hash_L24_T19": dict(image=1.2e-4, depth=1.1e-5, weights_sum=3.6e-6, grid=0.223, net=0.156, den=None, rgb=2.5e-2),
}
_HEADLINE_F16_LOOSE = dict(image=3e-2, depth=6e-2, weights_sum=3e-2, grid=0.25, net=0.25, den=0.25, rgb=0.25)   # used for a quantity whose pin is None


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("geom", ["hash_T19", "bear_tiled_T21", "hash_L24_T19"])
def test_run_end_to_end_vs_oracle_headline(geom, half):
    """1024 rays of a cfg2 view through run() + the reconstruction loss + backward with the headline field (hash L16 T = 2^19 desired 2048, and the
    reference field's own geometry: tiled L16 T = 2^21 desired 8192 — network_grid.py:89-96 —, and hash L24 T = 2^19: a 48-wide encoding, whose
    backward is the two-launch form), 64 + 64 samples, two hidden geometry layers —
    i.e. the fused samplers, BOTH gathers, the block-wise fused field, the indexed compositing, the fused field backward and the BINNED
    scatter (2.1 M (sample, level) pairs) in one piece, against oracle.torch_oracle.run on the CPU with the same parameters and RNG draws.
    renderer.py:278-474, network_grid.py:159-193."""
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider_utils import generate_rays
    tcnn.set_default_dtype(torch.float16 if half else torch.float32)
    try:
        gkw = dict(grid_type='tiledgrid', log2_hashmap_size=21, desired_resolution=8192) if geom == "bear_tiled_T21" else {}
        if geom == "hash_L24_T19":
            gkw = dict(num_levels=24)
        opt = sc.make_opt(fp16=half, **gkw)
        torch.manual_seed(0)
        model = NeRFNetwork(opt).cuda()
        ref = to.FieldRef(bound=opt.bound, num_levels=opt.num_levels, level_dim=2, base_resolution=16, log2_hashmap_size=opt.log2_hashmap_size,
                          desired_resolution=opt.desired_resolution, gridtype='tiled' if geom == "bear_tiled_T21" else 'hash', n_hidden_geo=2, half=half, seed=1)
        ref.pos_en.half = half
        g = torch.Generator().manual_seed(101)
        with torch.no_grad():
            ref.pos_en.embeddings.copy_((torch.rand(ref.pos_en.embeddings.shape, generator=g) * 2 - 1) * 0.5)     # visible features
            model.pos_en.embeddings.copy_(ref.pos_en.embeddings.cuda())
            model.pos_en.invalidate_half_table()
            model.network.params.copy_(ref.network.cuda())
            model.density_network.params.copy_(ref.density_network.cuda())
            model.rgb_network.params.copy_(ref.rgb_network.cuda())
        model.train()
        H = W = 128
        c2w = torch.from_numpy(sc.poses(8)).cuda()
        ro, rd = generate_rays(c2w[3:4], *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
        N = 1024
        sel = slice(60 * W, 60 * W + N)                                   # eight image rows through the middle of the view
        ro, rd = ro.view(-1, 3)[sel].contiguous(), rd.view(-1, 3)[sel].contiguous()
        g = torch.Generator().manual_seed(5)
        draws = dict(light=torch.randn(3, generator=g), z=torch.rand(N, 64, generator=g), u=torch.rand(N, 64, generator=g))
        kw = dict(num_steps=64, upsample_steps=64, perturb=True)
        r_ref = to.run(ref, ro.cpu(), rd.cpu(), torch.tensor([-2.0, -2, -2, 2, 2, 2]), opt.min_near, training=True, draws=draws, skip_fine_density=True, **kw)
        with torch.autocast('cuda', dtype=torch.float16, enabled=half):
            r = model.run(ro, rd, _draws=draws, **kw)
        rgb_gt, m_gt = sc.targets(1, 32, 32, seed=3)                      # 1024 target pixels

        def loss_of(res, dev):
            return ((res['image'].reshape(-1, 3).float() - rgb_gt[0].to(dev)) ** 2).mean() + 0.01 * ((res['render_mask'].reshape(-1).float() - m_gt[0].reshape(-1).to(dev)) ** 2).mean()
        l_ref, l = loss_of(r_ref, 'cpu'), loss_of(r, 'cuda')
        l_ref.backward()
        (l * (128.0 if half else 1.0)).backward()                         # a static loss scale for the half path (the gradients are compared un-scaled)
        inv = 1 / 128.0 if half else 1.0
        err = {}
        for k in ("image", "depth", "weights_sum"):
            err[k] = float(np.abs(r[k].detach().float().cpu().numpy() - r_ref[k].detach().numpy()).max())
        pairs = (("grid", model.pos_en.embeddings.grad, ref.pos_en.embeddings.grad), ("net", model.network.params.grad, ref.network.grad),
                 ("den", model.density_network.params.grad, ref.density_network.grad), ("rgb", model.rgb_network.params.grad, ref.rgb_network.grad))
        for name, a, b in pairs:
            b = b.numpy()
            assert float(np.abs(b).max()) > 0, name
            err[name] = float(np.abs(a.cpu().numpy() * inv - b).max() / np.abs(b).max())
        print(f"\nheadline parity [{geom}, {'f16' if half else 'f32'}]: loss {l.item():.6f} vs {l_ref.item():.6f}; " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
        if not half:
            for k in ("image", "depth", "weights_sum"):
                assert err[k] <= 1e-4, (k, err)
            np.testing.assert_allclose(r["weights"].detach().cpu().numpy(), r_ref["weights"].detach().numpy(), rtol=0, atol=1e-4)
            assert abs(l.item() - l_ref.item()) < 1e-5
            for name, a, b in pairs:
                b = b.numpy()
                # (as in the cfg1 test: the wave scans associate differently from torch's sequential cumprod / cumsum)
                np.testing.assert_allclose(a.cpu().numpy(), b, rtol=2e-3, atol=5e-4 * max(1e-3, float(np.abs(b).max())), err_msg=name)
        else:
            pin = _HEADLINE_F16_PIN[geom]
            for k, v in err.items():
                bound = pin[k] if pin[k] is not None else _HEADLINE_F16_LOOSE[k]
                assert v <= bound, (k, v, bound, err)
    finally:
        tcnn.set_default_dtype(torch.float32)
