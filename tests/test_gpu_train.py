"""GPU: the reconstruction step of the reference's trainer (utils_init_nerf.py:194-241, main.py:182-189) on the fused path
actually learns — loss on a learnable synthetic target drops — in fp32 and in fp16 (GradScaler policy on the device), the fused
Adam keeps the fp16 grid shadow in sync, and the device-side loss scaler follows torch.cuda.amp.GradScaler step for step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _target_scene(H, W, V):
    """A learnable target: colours of a smooth function of the ray direction, mask = central disc."""
    from customnerf_amd import scene as sc
    from customnerf_amd.nerf.provider_utils import generate_rays
    o, d = generate_rays(torch.from_numpy(sc.poses(V)).cuda(), *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
    o, d = o.view(V, 1, H * W, 3), d.view(V, 1, H * W, 3)
    rgb = (0.5 + 0.5 * torch.sin(d * 4.0)).view(V, H * W, 3)
    _, mask = sc.targets(V, H, W)
    return o, d, rgb.contiguous(), mask.cuda()


@pytest.mark.parametrize("fp16", [False, True], ids=["f32", "f16"])
def test_reconstruction_learns(fp16):
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16 if fp16 else torch.float32)
    try:
        torch.manual_seed(0)
        opt = sc.make_opt(fp16=fp16, num_levels=8, log2_hashmap_size=15, desired_resolution=256, lr=5e-3, iters=200)
        model = NeRFNetwork(opt).cuda()
        H = W = 32
        V = 4
        o, d, rgb, mask = _target_scene(H, W, V)
        tr = ReconTrainer(model, opt, fp16=fp16)
        losses = []
        for i in range(120):
            v = i % V
            loss, _ = tr.train_step(o[v], d[v], rgb[v], mask[v], num_steps=32, upsample_steps=32)
            losses.append(float(loss))
        first, last = np.mean(losses[:8]), np.mean(losses[-8:])
        assert np.isfinite(losses).all()
        assert last < 0.5 * first, (first, last)
        # parameters moved, gradients were zeroed by the fused step, no NaNs anywhere
        for n, p in model.named_parameters():
            assert torch.isfinite(p).all(), n
            assert torch.all(p.grad == 0), n
        if fp16:
            assert torch.equal(model.pos_en.half_table(), model.pos_en.embeddings.detach().half())
    finally:
        tcnn.set_default_dtype(torch.float16)


def test_march_path_step_runs_and_refreshes_occupancy():
    """`-O` path (run_cuda): occupancy refresh + a few training steps; sample counts come from the ray-ordered compaction."""
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)
    torch.manual_seed(0)
    opt = sc.make_opt(fp16=True, cuda_ray=True, num_levels=8, log2_hashmap_size=15, desired_resolution=256, lr=5e-3, iters=100)
    model = NeRFNetwork(opt).cuda()
    H = W = 32
    o, d, rgb, mask = _target_scene(H, W, 2)
    model.update_extra_state()                       # gaussian blob makes the centre dense -> non-empty bitfield
    assert int(model.density_bitfield.sum()) > 0
    tr = ReconTrainer(model, opt, fp16=True)
    for i in range(6):
        loss, out = tr.train_step(o[i % 2], d[i % 2], rgb[i % 2], mask[i % 2], dt_gamma=0, max_steps=256)
        assert np.isfinite(float(loss))
        rays = out['rays'].cpu().numpy()
        assert np.array_equal(rays[:, 0], np.arange(H * W))                       # ray-ordered
        assert np.array_equal(rays[1:, 1], np.cumsum(rays[:-1, 2]))               # exclusive scan of the counts
    model.update_extra_state()
    assert model.mean_count > 0


def test_train_one_epoch_on_a_disk_scene(tmp_path):
    """dataset front-end -> ReconTrainer via train_one_epoch (utils_init_nerf.py:577-671): loss goes down over epochs on a tiny scene"""
    import sys, os
    sys.path.insert(0, os.path.dirname(__file__))
    from test_provider import _write_scene
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider import NerfstudioScene
    from customnerf_amd.trainer import ReconTrainer, train_one_epoch
    _write_scene(str(tmp_path))
    views = NerfstudioScene(str(tmp_path), resolution_level=2, device="cuda")
    tcnn.set_default_dtype(torch.float16)
    torch.manual_seed(0)
    opt = sc.make_opt(fp16=True, num_levels=8, num_steps=16, upsample_steps=16, iters=200)
    model = NeRFNetwork(opt).cuda()
    tr = ReconTrainer(model, opt, fp16=True)
    logs = []
    losses = [train_one_epoch(tr, views, log=logs.append) for _ in range(4)]
    assert tr.global_step == 4 * len(views) and len(logs) == 4
    assert losses[-1] < losses[0] and all(np.isfinite(losses)), losses
    # view-parallel shard: rank 1 of 2 sees every second view
    before = tr.global_step
    train_one_epoch(tr, views, shard=(1, 2))
    assert tr.global_step - before == len(range(1, len(views), 2))
    # eval_step / test_step (utils_init_nerf.py:396-485): one unperturbed full-view render and the panels the reference writes out
    rgbs, mask, rays_o, rays_d, H, W, path = views[0]
    model.eval()
    panel, _, _, loss0 = tr.eval_step(views[0])
    n = 7 if opt.train_conf else 3
    assert panel.shape == (1, H, n * W, 3) and panel.dtype == torch.float32 and float(loss0) == 0.0
    assert torch.equal(panel[:, :, :W], rgbs.reshape(1, H, W, 3).float())
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
        out = model.render(rays_o, rays_d, staged=True, perturb=False, force_all_rays=True, num_steps=16, upsample_steps=16, dt_gamma=0, max_steps=opt.max_steps)
    assert torch.equal(panel[:, :, W:2 * W], out['image'].reshape(1, H, W, 3).float())
    assert torch.equal(panel[:, :, 2 * W:3 * W, 0], out['depth'].reshape(1, H, W).float())
    rgb_t, depth_t, d_t = tr.test_step(views[0])
    assert torch.equal(rgb_t, out['image'].reshape(1, H, W, 3).float()) and torch.equal(depth_t, out['depth'].reshape(1, H, W).float()) and int(d_t) == 0
    opt.render_all = True
    rgb_all, _, _ = tr.test_step(dict(rays_o=rays_o, rays_d=rays_d, H=H, W=W, dir=torch.tensor(2)), if_gui=True)
    assert rgb_all.shape == (1, H, (4 if opt.train_conf else 1) * W, 3)
    model.train()


def test_dynamic_loss_scaler_matches_torch_gradscaler():
    """optim.DynamicLossScaler + FusedAdam against torch.cuda.amp.GradScaler + torch.optim.Adam on the same gradient sequence with
    injected inf / NaN steps: same skipped steps, same scale trajectory (growth and backoff), same parameters (bias correction counts
    only the non-skipped steps)."""
    from customnerf_amd.optim import DynamicLossScaler, FusedAdam
    torch.manual_seed(0)
    shapes = [(70001,), (37, 16), (8,)]           # one tensor takes the per-tensor launch, two the multi-tensor launch (which also applies update())
    p_ref = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]
    p_our = [torch.nn.Parameter(p.detach().clone()) for p in p_ref]
    opt_ref = torch.optim.Adam([{'params': p_ref[:1], 'lr': 1e-2}, {'params': p_ref[1:], 'lr': 1e-3}], betas=(0.9, 0.99), eps=1e-15)
    opt_our = FusedAdam([{'params': p_our[:1], 'lr': 1e-2}, {'params': p_our[1:], 'lr': 1e-3}], betas=(0.9, 0.99), eps=1e-15)
    ref = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=4)
    ref.scale(torch.zeros(1, device="cuda"))                         # GradScaler creates its device state lazily
    our = DynamicLossScaler("cuda", init_scale=1024.0, growth_interval=4)
    opt_our.scaler = our
    from customnerf_amd.trainer import flat_grad_buffer, check_grads_finite
    flat = flat_grad_buffer(p_our)
    bad_steps = {3: float('inf'), 4: float('nan'), 11: float('-inf')}
    g = torch.Generator(device="cuda").manual_seed(1)
    for step in range(20):
        grads = [torch.randn(s, device="cuda", generator=g) for s in shapes]
        if step in bad_steps:
            grads[step % 3].view(-1)[5] = bad_steps[step]
        scale_ref = ref.get_scale()
        assert abs(our.get_scale() - scale_ref) < 1e-6 * scale_ref, (step, our.get_scale(), scale_ref)
        for p, q, gr in zip(p_ref, p_our, grads):
            p.grad = gr * scale_ref                                   # what backward of the scaled loss leaves behind
            q.grad.copy_(gr * scale_ref)
        ref.step(opt_ref)
        ref.update()
        opt_ref.zero_grad()
        check_grads_finite(our, p_our, flat)
        opt_our.step()
        assert opt_our.updates_scaler                                 # the small tensors' launch applied GradScaler.update() already
        our.update()                                                  # the standard idiom `opt.step(); scaler.update()` must not count the step twice
        for p, q in zip(p_ref, p_our):
            assert torch.all(q.grad == 0)
            assert torch.allclose(p, q, atol=1e-6, rtol=1e-5), (step, float((p - q).abs().max()))
    assert our.good_steps() == 20 - len(bad_steps)
    sd = our.state_dict()
    assert set(ref.state_dict()) <= set(sd) and sd["scale"] == ref.get_scale() and sd["_growth_tracker"] == ref.state_dict()["_growth_tracker"]
    again = DynamicLossScaler("cuda")
    again.load_state_dict(ref.state_dict())                          # a reference checkpoint's 'scaler' entry loads
    assert again.get_scale() == ref.get_scale()


@pytest.mark.parametrize("with_mask", [True, False])
def test_fused_recon_loss_matches_the_torch_formulation(with_mask):
    """cnerf_recon_loss (loss + gradient in one launch) against utils_init_nerf.py:220-234 written with F.mse_loss"""
    import torch.nn.functional as F
    from customnerf_amd.nerf.render_ops import recon_loss
    g = torch.Generator(device="cuda").manual_seed(0)
    N = 5000
    out_a = torch.rand(3, N, 6, device="cuda", generator=g).requires_grad_(True)
    out_b = out_a.detach().clone().requires_grad_(True)
    rgb, mask = torch.rand(N, 3, device="cuda", generator=g), (torch.rand(N, device="cuda", generator=g) > 0.5).float()
    la = recon_loss(out_a, rgb, mask if with_mask else None, 1.0, 0.3 if with_mask else 0.0)
    lb = F.mse_loss(out_b[0, :, 0:3], rgb) + (0.3 * F.mse_loss(out_b[0, :, 5], mask) if with_mask else 0.0)
    assert abs(float(la) - float(lb)) < 1e-6 * max(1.0, float(lb))
    (la * 7.0).backward(); (lb * 7.0).backward()
    assert torch.allclose(out_a.grad, out_b.grad, atol=1e-9, rtol=1e-5)
    assert bool((out_a.grad[1:] == 0).all())
    # the backward seed folded into the stored gradient (cnerf_recon_loss_scaled): the same bits as seeding afterwards, no multiply launch
    scale = torch.tensor([4096.0, 0.0, 0.0, 0.0], device="cuda")
    out_c, out_d = out_a.detach().clone().requires_grad_(True), out_a.detach().clone().requires_grad_(True)
    lc = recon_loss(out_c, rgb, mask if with_mask else None, 1.0, 0.3 if with_mask else 0.0, grad_scale=scale[0:1])
    lc.backward(gradient=scale[0].reshape(()))                       # DynamicLossScaler.backward's seed: the very scalar
    ld = recon_loss(out_d, rgb, mask if with_mask else None, 1.0, 0.3 if with_mask else 0.0)
    ld.backward(gradient=scale[0].reshape(()))
    assert torch.equal(out_c.grad, out_d.grad) and float(lc) == float(ld)
    out_e = out_a.detach().clone().requires_grad_(True)                # some other seed: the folded factor is corrected for
    (recon_loss(out_e, rgb, mask if with_mask else None, 1.0, 0.3 if with_mask else 0.0, grad_scale=scale[0:1]) * 3.0).backward()
    assert torch.allclose(out_e.grad, out_d.grad * (3.0 / 4096.0), rtol=1e-6, atol=0)


def test_multi_tensor_adam_matches_per_tensor_launches():
    """cnerf_adam_step_scaled_multi (the three MLP vectors in one single-workgroup launch, GradScaler.update() in its tail) against
    cnerf_adam_step_scaled per tensor + cnerf_scaler_update: the same bits, with and without an overflow step."""
    from customnerf_amd import optim
    from customnerf_amd.optim import DynamicLossScaler, FusedAdam
    g = torch.Generator(device="cuda").manual_seed(3)
    shapes = [(10240,), (5120,), (7168,), (13,)]
    for bad in (False, True):
        runs = []
        for small_max in (1 << 16, 0):                                # multi-tensor path on / off
            old = optim.SMALL_PARAM_MAX
            optim.SMALL_PARAM_MAX = small_max
            try:
                gg = torch.Generator(device="cuda").manual_seed(5)
                ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gg)) for s in shapes]
                opt = FusedAdam([{'params': ps[:2], 'lr': 1e-2}, {'params': ps[2:], 'lr': 1e-3}], betas=(0.9, 0.99), eps=1e-15)
                sc = DynamicLossScaler("cuda", init_scale=256.0, growth_interval=2)
                opt.scaler = sc
                for step in range(5):
                    for p in ps:
                        p.grad = torch.randn(p.shape, device="cuda", generator=gg) * 256.0
                    if bad and step == 2:
                        ps[1].grad[7] = float("inf")
                    for p in ps:
                        sc.check(p.grad)
                    opt.step()
                    sc.update()                                       # applies it, or does nothing when the step's last launch already has
                    assert opt.updates_scaler == (small_max > 0)
                runs.append(([p.detach().clone() for p in ps], sc.state.clone()))
            finally:
                optim.SMALL_PARAM_MAX = old
        for a, b in zip(runs[0][0], runs[1][0]):
            assert torch.equal(a, b)
        assert torch.equal(runs[0][1], runs[1][1])


def test_in_place_gradient_accumulation_matches_autograd_accumulation():
    """The trainers let the grid scatter and the field's weight-gradient reduction add straight into the persistent .grad buffers
    (GridEncoder.grad_in_place / NeRFNetwork.grad_in_place, trainer.enable_grad_in_place).  Same draws, same loss: the gradients must equal
    what autograd's AccumulateGrad produces on the plain path — and accumulate over two backward passes the same way."""
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import enable_grad_in_place, flat_grad_buffer
    tcnn.set_default_dtype(torch.float16)
    try:
        H = W = 32
        o, d, rgb, mask = _target_scene(H, W, 1)
        g = torch.Generator().manual_seed(7)
        draws = dict(light=torch.randn(3, generator=g), z=torch.rand(H * W, 32, generator=g), u=torch.rand(H * W, 32, generator=g))
        grads = []
        for in_place in (False, True):
            torch.manual_seed(0)
            opt = sc.make_opt(fp16=True, num_levels=16, log2_hashmap_size=19, desired_resolution=2048)
            model = NeRFNetwork(opt).cuda().train()
            with torch.no_grad():
                model.pos_en.embeddings.uniform_(-0.3, 0.3)
            flat = flat_grad_buffer(model.parameters())                 # persistent zeroed .grad views in both runs
            if in_place:
                enable_grad_in_place(model)
            for _ in range(2):                                          # two passes: the second must ADD to the first
                with torch.autocast('cuda', dtype=torch.float16):
                    res = model.render(o[0], d[0], staged=False, perturb=True, force_all_rays=True, num_steps=32, upsample_steps=32, _draws=draws)
                    loss = ((res['image'].reshape(-1, 3).float() - rgb[0]) ** 2).mean() + 0.1 * res['render_mask'].float().mean()
                (loss * 1024.0).backward()
            assert all(p.grad.data_ptr() >= flat.data_ptr() for p in model.parameters())      # the views stayed bound
            grads.append([p.grad.clone() for p in model.parameters()])
        for a, b in zip(*grads):
            assert float(b.abs().max()) > 0
            # grid: exact fixed-point sums either way, but the plain path rounds each pass to float32 before adding: rounding-level difference
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))
    finally:
        tcnn.set_default_dtype(torch.float32)


def test_in_place_gradients_from_two_streams_are_ordered():
    """_lib.grad_chain_wait / _record: the in-place gradient producers of one stream enqueue nothing (launch order is the order); a producer on a
    second stream orders itself after the first stream's tail.  Two passes — the second on a side stream that does NOT wait for the main stream
    by itself — accumulate the gradients of two passes on one stream."""
    from customnerf_amd import scene as sc, tcnn, _lib
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import enable_grad_in_place, flat_grad_buffer
    tcnn.set_default_dtype(torch.float16)
    try:
        H = W = 64
        o, d, rgb, mask = _target_scene(H, W, 1)
        g = torch.Generator().manual_seed(7)
        draws = dict(light=torch.randn(3, generator=g), z=torch.rand(H * W, 32, generator=g), u=torch.rand(H * W, 32, generator=g))
        grads = []
        for two_streams in (False, True):
            torch.manual_seed(0)
            opt = sc.make_opt(fp16=True, num_levels=16, log2_hashmap_size=19, desired_resolution=2048)
            model = NeRFNetwork(opt).cuda().train()
            flat = flat_grad_buffer(model.parameters())
            enable_grad_in_place(model)

            def one_pass():
                with torch.autocast('cuda', dtype=torch.float16):
                    res = model.render(o[0], d[0], staged=False, perturb=True, force_all_rays=True, num_steps=32, upsample_steps=32, _draws=draws)
                    loss = ((res['image'].reshape(-1, 3).float() - rgb[0]) ** 2).mean() + 0.1 * res['render_mask'].float().mean()
                (loss * 1024.0).backward()

            with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):      # settle the per-model caches (fp16 shadow table) ...
                model.render(o[0], d[0], staged=False, perturb=True, force_all_rays=True, num_steps=32, upsample_steps=32, _draws=draws)
            torch.cuda.synchronize()                                                 # ... so that the side stream's forward reads nothing in flight
            one_pass()
            if two_streams:
                side = torch.cuda.Stream()
                with torch.cuda.stream(side):                            # (no side.wait_stream(main): the producers have to order themselves)
                    one_pass()
                assert _lib._GRAD_CHAIN[o.device].cuda_stream == side.cuda_stream
                torch.cuda.current_stream().wait_stream(side)
            else:
                one_pass()
            torch.cuda.synchronize()
            grads.append([p.grad.clone() for p in model.parameters()])
        for a, b in zip(*grads):
            assert float(a.abs().max()) > 0 and torch.equal(a, b)
    finally:
        tcnn.set_default_dtype(torch.float32)


def test_training_is_bit_reproducible():
    """Two identical fp16 trainings (same seed, full-size 128x128 views so that the binned fixed-point scatter, the wave-specialised field
    backward and the split-bin reduction all run) end in bit-identical parameters: every reduction on the path has a fixed order or is
    exact (the reference's half2 atomic scatter is not reproducible)."""
    _check_training_is_bit_reproducible(16)


def test_training_is_bit_reproducible_at_24_levels():
    """the same with a 24-level table: the two-launch field backward and its split-K partial rows"""
    _check_training_is_bit_reproducible(24)


def _check_training_is_bit_reproducible(num_levels):
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)

    def train():
        torch.manual_seed(0)
        opt = sc.make_opt(fp16=True, num_levels=num_levels)
        model = NeRFNetwork(opt).cuda()
        H = W = 128
        V = 2
        o, d, rgb, mask = _target_scene(H, W, V)
        tr = ReconTrainer(model, opt, fp16=True)
        for i in range(3):
            tr.train_step(o[i % V], d[i % V], rgb[i % V], mask[i % V], num_steps=opt.num_steps, upsample_steps=opt.upsample_steps)
        return [p.detach().clone() for p in model.parameters()]

    try:
        a, b = train(), train()
    finally:
        tcnn.set_default_dtype(torch.float32)                 # the fp16 default must not leak into later tests
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb)


def test_training_is_bit_identical_with_and_without_packed_weights():
    """the trainers run their steps on the packed fp16 image of the MLP parameters (trainer.packed_weights_window: one pack per optimiser step
    instead of staging in each of the three field launches); six steps — eager, then the graphed step, whose capture records its own pack —
    end in the parameters of the same steps with the image off (`opt.packed_field_weights = False`), bit for bit"""
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)

    def train(packed):
        torch.manual_seed(0)
        opt = sc.make_opt(fp16=True)
        opt.packed_field_weights = packed
        model = NeRFNetwork(opt).cuda()
        H = W = 64
        o, d, rgb, mask = _target_scene(H, W, 1)
        tr = ReconTrainer(model, opt, fp16=True)
        kw = dict(num_steps=opt.num_steps, upsample_steps=opt.upsample_steps)
        for i in range(3):
            torch.manual_seed(100 + i)
            tr.train_step(o[0], d[0], rgb[0], mask[0], **kw)
        used = bool(model.__dict__.get('_wimg_cache'))
        assert not model.__dict__.get('packed_field_weights', False)        # the window closed with the step
        for i in range(4):                                                  # (two eager warm-ups + capture + one replay inside)
            torch.manual_seed(200 + i)
            tr.train_step_graphed(o[0], d[0], rgb[0], mask[0], **kw)
        return [p.detach().clone() for p in model.parameters()], used

    try:
        (a, used_a), (b, used_b) = train(True), train(False)
    finally:
        tcnn.set_default_dtype(torch.float32)
    assert used_a and not used_b
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb)


def test_training_without_the_unused_composites_is_bit_identical():
    """ReconTrainer renders with fg_bg=False (its loss reads the first composite; the edit-region / background composites are not computed): the
    parameters after four steps are those of the same steps with all three composites (`needs_fg_bg = True`), and the outputs have no 'fg'"""
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)

    def train(need):
        torch.manual_seed(0)
        opt = sc.make_opt(fp16=True)
        model = NeRFNetwork(opt).cuda()
        o, d, rgb, mask = _target_scene(64, 64, 1)
        tr = ReconTrainer(model, opt, fp16=True)
        tr.needs_fg_bg = need
        for i in range(4):
            torch.manual_seed(100 + i)
            _, outputs = tr.train_step(o[0], d[0], rgb[0], mask[0], num_steps=opt.num_steps, upsample_steps=opt.upsample_steps)
        return [p.detach().clone() for p in model.parameters()], ('fg' in outputs)

    try:
        (a, fa), (b, fb) = train(False), train(True)
    finally:
        tcnn.set_default_dtype(torch.float32)
    assert not fa and fb
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb)


def test_training_is_bit_identical_with_the_table_step_inside_the_scatter():
    """ReconTrainer arms the grid table's Adam update for its one backward pass (optim.FusedAdam.arm_in_backward -> cnerf_grid_backward_adam): eight
    steps — among them one the loss scaler skips (its scale is raised until the half-precision gradients overflow) — end in the parameters, Adam
    moments and scaler state of the same steps with `opt.fuse_table_adam = False`, bit for bit; and the fused run really took the fused path"""
    _check_table_step_inside_the_scatter(16)


def test_training_is_bit_identical_with_the_table_step_inside_the_scatter_at_24_levels():
    """the same with a 24-level table (the field backward's two-launch form raises found_inf for the folded check)"""
    _check_table_step_inside_the_scatter(24)


def _check_table_step_inside_the_scatter(num_levels):
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)

    def train(fuse):
        torch.manual_seed(0)
        opt = sc.make_opt(fp16=True, num_levels=num_levels)
        opt.fuse_table_adam = fuse
        model = NeRFNetwork(opt).cuda()
        H = W = 64
        o, d, rgb, mask = _target_scene(H, W, 1)
        tr = ReconTrainer(model, opt, fp16=True)
        kw = dict(num_steps=opt.num_steps, upsample_steps=opt.upsample_steps)
        applied = []
        inner = tr.optimizer.disarm_in_backward
        tr.optimizer.disarm_in_backward = lambda: (applied.append(inner()), applied[-1])[1]
        for i in range(8):
            torch.manual_seed(100 + i)
            if i == 4:
                tr.scaler.state[0] = 2.0 ** 40                              # this step overflows: skipped, the scale backs off
            tr.train_step(o[0], d[0], rgb[0], mask[0], **kw)
            if i == 4:
                tr.scaler.state[0] = 65536.0
        emb = model.pos_en.embeddings
        st = tr.optimizer.state[emb]
        n_applied = sum(a is not None for a in applied)
        return ([p.detach().clone() for p in model.parameters()] + [st['exp_avg'].clone(), st['exp_avg_sq'].clone(), tr.scaler.state.clone(),
                                                                    model.pos_en.half_table().clone()], n_applied, st['step'])

    try:
        (a, na, sa), (b, nb, sb) = train(True), train(False)
    finally:
        tcnn.set_default_dtype(torch.float32)
    assert na == 8 and nb == 0 and sa == sb == 8
    assert float(a[-2][3]) == 7.0                                           # seven counted steps: the overflowing one was skipped in both runs
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb)


def test_training_trajectory_is_bit_identical_with_and_without_early_termination():
    """Early termination (the compositing backward flushes gradients the half-precision consumers would round to zero; field backward and scatter skip the
    dead tiles / rows) is claimed to change no bit of any parameter gradient.  Compounded over a run: 400 optimiser steps on the analytic sphere scene from
    one seed, with and without it — while the loss falls by two orders of magnitude, most rows die and the scatter's bins crowd — end in bit-identical
    parameters (profiles/r05_early_termination_trajectory.log is the 1200-step version, scratch/soak_early_term.py)."""
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider_utils import generate_rays
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)
    H = W = 128
    V = 8

    def train(early):
        torch.manual_seed(0)
        opt = sc.make_opt(cuda_ray=False, fp16=True)
        opt.early_termination = early
        model = NeRFNetwork(opt).cuda()
        c2w = torch.from_numpy(sc.poses(V)).cuda()
        o, d = generate_rays(c2w, *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
        o, d = o.view(V, 1, H * W, 3), d.view(V, 1, H * W, 3)
        rgb, mask = sc.sphere_targets(o.reshape(V, -1, 3), d.reshape(V, -1, 3))
        tr = ReconTrainer(model, opt, fp16=True)
        first = last = None
        for i in range(400):
            loss, _ = tr.train_step(o[i % V], d[i % V], rgb[i % V], mask[i % V], num_steps=opt.num_steps, upsample_steps=opt.upsample_steps)
            if i == 0:
                first = float(loss)
            last = float(loss)
        return [p.detach().clone() for p in model.parameters()], first, last

    try:
        (a, f0, l0), (b, f1, l1) = train(True), train(False)
    finally:
        tcnn.set_default_dtype(torch.float32)
    assert f0 == f1 and l0 == l1 and l0 < 0.02 * f0, (f0, l0, f1, l1)       # it did train (and identically)
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb)


def test_half_batches_sum_to_the_full_batch():
    """SURVEY.md §4's data-parallel contract on the real field, on one GPU: the gradient of a ray batch equals the sum of the gradients of its
    two halves (each weighted by its share of the rays) — what two ranks of a ray-chunk split produce before the exchange.  Full-size view
    (128 x 128, L16 T2^19, 64 + 64 samples, fp16) so that the binned fixed-point scatter, the x2 field backward and the fused loss all run.
    The per-sample table updates are identical in both runs and each launch sums them exactly (64-bit fixed point); what differs is ONE float32
    rounding per entry when a launch's sum is added to `.grad` (once for the full batch, twice for the halves): the table gradients agree to
    float32 rounding, not bit for bit; the MLP gradients (float32 partial sums in a different order) to 1e-5 of their scale."""
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)
    try:
        torch.manual_seed(0)
        opt = sc.make_opt(fp16=True)
        model = NeRFNetwork(opt).cuda()
        with torch.no_grad():
            model.pos_en.embeddings.uniform_(-0.3, 0.3)
            model.pos_en.invalidate_half_table()
        H = W = 128
        o, d, rgb, mask = _target_scene(H, W, 1)
        N = H * W
        tr = ReconTrainer(model, opt, fp16=True)
        g = torch.Generator().manual_seed(5)
        draws = dict(z=torch.rand(N, 64, generator=g).cuda(), u=torch.rand(N, 64, generator=g).cuda())
        model.train()

        def grad_of(lo, hi, weight):
            dr = dict(z=draws['z'][lo:hi].contiguous(), u=draws['u'][lo:hi].contiguous())
            with torch.autocast('cuda', dtype=torch.float16):
                out = model.render(o[0][:, lo:hi].contiguous(), d[0][:, lo:hi].contiguous(), staged=False, perturb=True, force_all_rays=True,
                                   num_steps=64, upsample_steps=64, _draws=dr)
                loss = tr.loss(out, rgb[0][lo:hi].contiguous(), mask[0][lo:hi].contiguous())
            tr.scaler.backward(loss * weight)                           # weight = this chunk's share of the rays (a power of two: exact)

        def take():
            gs = [p.grad.detach().clone() for p in model.parameters()]
            for p in model.parameters():
                p.grad.zero_()
            return gs

        grad_of(0, N, 1.0)
        full = take()
        grad_of(0, N // 2, 0.5)
        grad_of(N // 2, N, 0.5)
        halves = take()
        names = [n for n, _ in model.named_parameters()]
        for n, a, b in zip(names, full, halves):
            scale = float(a.abs().max())
            assert scale > 0, n
            if n == "pos_en.embeddings":
                assert float((a != 0).float().mean()) > 0.01
                np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=3e-7, atol=2e-7 * scale, err_msg=n)
            else:
                np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=0, atol=1e-5 * scale, err_msg=n)
    finally:
        tcnn.set_default_dtype(torch.float32)


def test_sharded_exchange_on_the_gpu_single_rank():
    """customnerf_amd.dp.ShardedExchange on the real device path (RCCL process group of ONE rank: the collectives are self-copies, everything else is the
    code an 8-GPU run executes): float16 payload, float32 sum on arrival, `cnerf_adam_step_scaled` on the padded owner shard, in-place all-gather of the
    float16 shadow, found-inf check + MAX all-reduce, the MLP all-reduce started from the pre-scatter hook.
    Step 1 is checked exactly: the table after the step == Adam (spelled out in torch) on float(half(gradient)) — the payload's float16 rounding is the
    only arithmetic difference from the plain trainer (with eps = 1e-15 Adam turns a flushed-to-zero gradient into a full-size step difference, which is
    why the two trainers are not compared entry by entry).  Then the loss of a few steps is compared with the plain fused-Adam trainer."""
    import os
    import torch.distributed as dist
    from customnerf_amd import scene as sc, tcnn, dp as dpm
    from customnerf_amd.gridencoder import grid as ge
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer, setup_sharded_dp
    tcnn.set_default_dtype(torch.float16)
    created = False
    try:
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29541")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
            created = True
        H = W = 128
        o, d, rgb, mask = _target_scene(H, W, 2)
        losses = {}
        for mode in ("plain", "sharded"):
            torch.manual_seed(0)
            opt = sc.make_opt(fp16=True)
            model = NeRFNetwork(opt).cuda()
            tr = ReconTrainer(model, opt, fp16=True)
            table = model.pos_en.embeddings
            fired, seen = [], {}
            if mode == "sharded":
                tr._dp = setup_sharded_dp(tr, model, True, rank=0)
                st = tr._dp.state[0]
                assert len(tr._dp.state) == 1 and st['shard'] % 64 == 0 and st['p'] is table
                assert model.pos_en.half_table().data_ptr() == tr._dp.shadow_table(table).data_ptr()
                start, exchange = tr._dp.start_small, tr._dp.exchange

                def start_small():
                    fired.append(1)
                    start()

                def exchange_and_keep():
                    if 'g' not in seen:
                        seen['g'] = tr._flat[st['off']:st['off'] + st['n']].clone()
                        seen['p0'] = st['master'][:st['n']].clone()
                        seen['scale'] = float(tr.scaler.state[0])
                    exchange()
                tr._dp.start_small, tr._dp.exchange = start_small, exchange_and_keep
                ge.set_pre_scatter_hook(start_small)
            ls = []
            for i in range(4):
                torch.manual_seed(100 + i)
                out = tr.train_step(o[i % 2], d[i % 2], rgb[i % 2], mask[i % 2], num_steps=opt.num_steps, upsample_steps=opt.upsample_steps)
                ls.append(float(out[0] if isinstance(out, (tuple, list)) else out))
                if mode == "sharded" and i == 0:
                    g16 = seen['g'].half().float()                         # the payload (world 1: pre-scale 1)
                    assert float(seen['g'].abs().max()) > 0
                    p, m, v = seen['p0'].clone(), torch.zeros_like(g16), torch.zeros_like(g16)
                    lr = tr._dp.lr_of(table)                                # lr factor of step 0 is 1
                    dpm._adam_host(p, g16, m, v, None, lr, (0.9, 0.99), 1e-15, 1, 1.0 / seen['scale'])
                    got = st['master'][:st['n']]
                    assert float((got - p).abs().max()) <= 2e-6 * lr + 1e-9, float((got - p).abs().max())
                    assert float((got - seen['p0']).abs().max()) > 0.5 * lr          # it did step
                    assert torch.equal(tr._dp.shadow_table(table).reshape(-1), got.half())      # shadow shard == half(master shard), gathered in place
                    assert float(tr._flat[st['off']:st['off'] + st['n']].abs().max()) == 0        # the scatter target was re-zeroed
            if mode == "sharded":
                assert len(fired) >= 4                                    # the hook fired in every backward
                tr._dp.consolidate()
                assert torch.equal(tr._dp.shadow_table(table), table.detach().half())
                assert tr.scaler.good_steps() == 4
                assert all(bool(torch.isfinite(q).all()) for q in model.parameters())
            losses[mode] = ls
            ge.set_pre_scatter_hook(None)
        assert abs(losses["plain"][0] - losses["sharded"][0]) <= 1e-6 * abs(losses["plain"][0])         # same start
        for a, b in zip(losses["plain"], losses["sharded"]):
            assert abs(a - b) <= 0.1 * abs(a), (losses)
    finally:
        ge.set_pre_scatter_hook(None)
        if created:
            dist.destroy_process_group()
        tcnn.set_default_dtype(torch.float32)


@pytest.mark.parametrize("n,world", [(1000003, 8), (4096, 2), (65, 1)])
def test_dp_pack_and_reduce_kernels(n, world):
    """cnerf_dp_pack / cnerf_dp_reduce against the torch spelling dp.ShardedExchange uses on host tensors: half(g * 1/world) with the source zeroed;
    float32 sum of the world float16 slices, found-inf raised for a non-finite sum only."""
    from customnerf_amd._lib import lib, check, ptr, stream
    g = torch.Generator(device="cuda"); g.manual_seed(n)
    base = torch.randn(n + 4, device="cuda", generator=g) * 100.0
    grad = base[4:]                                                       # 16-byte aligned view at an offset, ragged tail
    want = (grad * (1.0 / world)).half()
    payload = torch.full((n + 8,), 7.0, dtype=torch.float16, device="cuda")
    check(lib.cnerf_dp_pack(ptr(grad), ptr(payload), n, 1.0 / world, stream()), "dp_pack")
    assert torch.equal(payload[:n], want) and float(payload[n:].min()) == 7.0
    assert float(grad.abs().max()) == 0 and float(base[:4].abs().min()) > 0
    shard = (n // world + 63) // 64 * 64
    recv = (torch.randn(world, shard, device="cuda", generator=g) * 50.0).half()
    out = torch.empty(shard, device="cuda")
    state = torch.tensor([65536.0, 0, 0, 0], device="cuda")
    check(lib.cnerf_dp_reduce(ptr(recv), world, shard, ptr(out), ptr(state), stream()), "dp_reduce")
    ref = torch.zeros(shard, device="cuda")
    for r in range(world):
        ref += recv[r].float()                                            # same order: sequential float32 adds
    assert torch.equal(out, ref) and float(state[2]) == 0.0
    recv[world - 1, shard - 1] = float("inf")
    check(lib.cnerf_dp_reduce(ptr(recv), world, shard, ptr(out), ptr(state), stream()), "dp_reduce")
    assert float(state[2]) == 1.0 and torch.isinf(out[-1])
    assert lib.cnerf_dp_reduce(ptr(recv), world, shard + 8, ptr(out), None, stream()) < 0      # shard not a multiple of 64: rejected


@pytest.mark.parametrize("tag", ["conf", "conf2", "batch"])
def test_recon_step_matches_reference_golden(tag):
    """ReconTrainer.loss on the fused renderer (cnerf_composite_run + the one-launch loss kernel and its gradient) replaying the reference's own
    Trainer_Nerf.train_step_pretrain (nerf/utils_init_nerf.py:194-241; tests/golden/editing.npz): image, loss and the gradient of the toy field's
    six parameters."""
    import argparse
    import os
    from customnerf_amd import scene as sc
    from customnerf_amd.nerf.renderer import NeRFRenderer
    from customnerf_amd.trainer import ReconTrainer
    from oracle.toy_field import ToyField
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "editing.npz"))
    T = lambda a: torch.from_numpy(np.asarray(a)).cuda()
    opt = sc.make_opt(fp16=False, num_steps=int(g["opt__num_steps"]), upsample_steps=int(g["opt__upsample_steps"]), min_near=float(g["opt__min_near"]),
                      train_conf=float(g[f"pre_{tag}__train_conf"]), train_rgb=float(g[f"pre_{tag}__train_rgb"]))

    class ToyParam(NeRFRenderer):
        def __init__(self, opt, theta):
            super().__init__(opt)
            self.theta = torch.nn.Parameter(theta.clone())
            self.f = ToyField(self.theta)

        def forward(self, x, d, *a, **k):
            return self.f(x, d)

        def density(self, x):
            return self.f.density(x)
    model = ToyParam(opt, T(g["theta_edit"])).cuda().train()
    draws = dict(light=T(g[f"pre_{tag}__light"]), z=T(g[f"pre_{tag}__z"]), u=T(g[f"pre_{tag}__u"]))
    # "batch": --batch_rays subsampling (utils_init_nerf.py:210-215) through ReconTrainer.select_rays, replaying the reference's recorded np.random.choice draw
    opt.batch_rays = int(g[f"pre_{tag}__batch_rays"])
    shim = argparse.Namespace(opt=opt)
    rays_o, rays_d, rgbs, mask = ReconTrainer.select_rays(shim, T(g["rays_o"]), T(g["rays_d"]), T(g["rgbs"]), T(g["mask"]),
                                                          g[f"pre_{tag}__select_inds"] if opt.batch_rays else None)
    assert rays_o.reshape(-1, 3).shape[0] == (opt.batch_rays or int(g["H"]) * int(g["W"]))
    out = model.render(rays_o, rays_d, staged=False, perturb=True, force_all_rays=True, _draws=draws, **{k: v for k, v in vars(opt).items() if k != "bg_color"})
    assert "_out_ray" in out                                                   # the fused path: the loss below is the one-launch kernel
    loss = ReconTrainer.loss(shim, out, rgbs, mask)
    loss.backward()
    print(f"[pretrain golden {tag}] image max|diff| {np.abs(out['image'].detach().cpu().numpy() - g[f'pre_{tag}__pred_rgb']).max():.3e}")
    np.testing.assert_allclose(out["image"].detach().cpu().numpy(), g[f"pre_{tag}__pred_rgb"], rtol=0, atol=1e-5)      # north_star asks 1e-4 fp32; measured 1.5e-7
    np.testing.assert_allclose(float(loss.detach()), float(g[f"pre_{tag}__loss"]), rtol=2e-4)
    want = g[f"pre_{tag}__grad_theta"]
    assert np.abs(model.theta.grad.cpu().numpy() - want).max() <= 2e-3 * np.abs(want).max(), (model.theta.grad.cpu().numpy(), want)


def test_train_step_graphed_follows_the_eager_trainer():
    """ReconTrainer.train_step_graphed (render + loss + backward as one hipGraph per view, eager optimiser step): the same training as train_step —
    different random jitter, so the comparison is the loss trajectory — and bit-reproducible from run to run"""
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider_utils import generate_rays
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)
    H = W = 64                                      # >= 2^20 (sample, level) pairs per backward: the bit-reproducible binned scatter, not the float-atomic kernel
    V = 2
    c2w = torch.from_numpy(sc.poses(V)).cuda()
    ro, rd = generate_rays(c2w, *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
    ro, rd = ro.view(V, 1, H * W, 3), rd.view(V, 1, H * W, 3)
    rgb, mask = sc.targets(V, H, W)
    rgb, mask = rgb.cuda(), mask.cuda()
    views = [(ro[v].contiguous(), rd[v].contiguous(), rgb[v].contiguous(), mask[v].contiguous()) for v in range(V)]

    def run(graphed, steps=12):
        torch.manual_seed(0)
        opt = sc.make_opt(fp16=True, num_steps=16, upsample_steps=16, iters=100)
        model = NeRFNetwork(opt).cuda()
        tr = ReconTrainer(model, opt, fp16=True)
        kw = dict(num_steps=16, upsample_steps=16, dt_gamma=0, max_steps=opt.max_steps)
        losses = []
        for i in range(steps):
            step = tr.train_step_graphed if graphed else tr.train_step
            loss, _ = step(*views[i % V], **kw)
            losses.append(float(loss))
        return losses, [p.detach().clone() for p in model.parameters()], tr
    le, _, _ = run(False, steps=16)                     # (the graphed trainer spends two eager steps + the captured one per view on its first visit)
    lg, pg, trg = run(True)
    lg2, pg2, _ = run(True)
    assert trg.global_step == 12 + 2 * V and len(trg._graphs) == V
    assert all(np.isfinite(lg)) and lg[-1] < lg[0] and abs(lg[-1] - le[-1]) < 0.15 * le[-1], (le, lg)
    assert lg == lg2 and all(torch.equal(a, b) for a, b in zip(pg, pg2))
    with pytest.raises(ValueError):
        opt2 = sc.make_opt(fp16=False, num_levels=8)
        ReconTrainer(NeRFNetwork(opt2).cuda(), opt2, fp16=False).train_step_graphed(*views[0], num_steps=16, upsample_steps=16, dt_gamma=0, max_steps=1024)

@pytest.mark.gpu
def test_graphed_step_owns_its_buffers():
    """a captured graph must not read buffers whose lifetime it does not control.  (1) more views than the renderer's 64-entry
    [d | d] cache holds: the concatenation is a node of the graph (its result lives in the graph pool), so replaying view 0 after 70 other views is
    still the training the eager trainer does, run after run bit-identical; (2) a grow-on-demand workspace reallocated by an interleaved larger
    eager step (scratch generation) drops every cached graph and the next visit recaptures."""
    from customnerf_amd import scene as sc, tcnn, _lib
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider_utils import generate_rays
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)
    from customnerf_amd import field as fld
    from customnerf_amd.gridencoder import grid as ge
    ge._WS_CACHE.clear(); fld._WS.clear()              # earlier tests of the session may have left large workspaces: (2) needs a real growth
    H = W = 16
    V = 70

    def make_views(V, H, W):
        c2w = torch.from_numpy(sc.poses(V)).cuda()
        ro, rd = generate_rays(c2w, *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
        ro, rd = ro.view(V, 1, H * W, 3), rd.view(V, 1, H * W, 3)
        rgb, mask = sc.targets(V, H, W)
        rgb, mask = rgb.cuda(), mask.cuda()
        return [(ro[v].contiguous(), rd[v].contiguous(), rgb[v].contiguous(), mask[v].contiguous()) for v in range(V)]
    views = make_views(V, H, W)
    kw = dict(num_steps=8, upsample_steps=8, dt_gamma=0, max_steps=1024)

    def run(graphed):
        torch.manual_seed(0)
        opt = sc.make_opt(fp16=True, num_levels=8, num_steps=8, upsample_steps=8, iters=1000)
        model = NeRFNetwork(opt).cuda()
        tr = ReconTrainer(model, opt, fp16=True)
        losses = []
        for epoch in range(2):
            for v in range(V):
                loss, _ = (tr.train_step_graphed if graphed else tr.train_step)(*views[v], **kw)
                losses.append(float(loss))
        return losses, tr, model
    lg, trg, model = run(True)
    le, _, _ = run(False)
    assert len(trg._graphs) == V and len(model._dirs2_cache) <= 64
    assert all(np.isfinite(lg))                                          # (float-atomic scatter at this size: not bit-reproducible, so compare with the eager trainer)
    assert abs(np.mean(lg[V:]) - np.mean(le[V:])) < 0.1 * np.mean(le[V:]), (np.mean(lg[V:]), np.mean(le[V:]))
    # under capture the [d | d] concatenation is a graph node with its result in the graph pool, not a cache entry
    n_cached = len(model._dirs2_cache)
    fresh = views[0][1].view(-1, 3).clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d2 = model._dirs_twice(fresh)
    g.replay()
    torch.cuda.synchronize()
    assert len(model._dirs2_cache) == n_cached and torch.equal(d2, torch.cat([fresh, fresh], 0))
    # (2) an eager step on a larger view grows the backward workspaces: the graphs captured before it are dropped, not replayed
    gen = _lib.scratch_generation()
    big = make_views(1, 128, 128)[0]                                    # >= 2^20 (sample, level) pairs: the binned scatter's workspaces (side-stream plan + records)
    trg.train_step(*big, **kw)
    assert _lib.scratch_generation() > gen
    step0 = trg.global_step
    loss, _ = trg.train_step_graphed(*views[0], **kw)
    assert len(trg._graphs) == 1 and trg.global_step == step0 + 3 and np.isfinite(float(loss))
    loss, _ = trg.train_step_graphed(*views[0], **kw)                    # and the recaptured graph replays
    assert len(trg._graphs) == 1 and trg.global_step == step0 + 4 and np.isfinite(float(loss))
    # (3) ADVICE r5: the workspaces a graph references are keyed by the CAPTURE stream and grown inside a capture.  A larger view captured
    # after a smaller one re-grows them in its own capture (the eager stream's are big enough since (2), so its warm-up moves nothing): the
    # smaller view's graph — which holds the old block, now back in the shared graph pool — must be dropped, not replayed.
    # 96 x 96 rays x 16 samples x 8 levels >= 2^20 pairs: the binned scatter's workspace, first allocated under the capture stream here ...
    mid = make_views(1, 96, 96)[0]
    loss, _ = trg.train_step_graphed(*mid, **kw)
    assert np.isfinite(float(loss)) and 1 <= len(trg._graphs) <= 2
    # ... and outgrown (1.25 x head-room: 9216 -> 11520 rays) by a 120 x 120 view's capture
    gen = _lib.scratch_generation()
    big2 = make_views(1, 120, 120)[0]
    loss, _ = trg.train_step_graphed(*big2, **kw)
    assert _lib.scratch_generation() > gen                               # grown during this view's capture
    assert len(trg._graphs) == 1 and np.isfinite(float(loss))            # every graph captured before is gone, the new one stays
    step0 = trg.global_step
    loss, _ = trg.train_step_graphed(*mid, **kw)                         # recaptures (two eager steps + the captured one) against the grown buffers
    assert len(trg._graphs) == 2 and trg.global_step == step0 + 3 and np.isfinite(float(loss))
    for _ in range(2):                                                   # both replay side by side from now on
        la, _ = trg.train_step_graphed(*big2, **kw)
        lb, _ = trg.train_step_graphed(*mid, **kw)
        assert len(trg._graphs) == 2 and np.isfinite(float(la)) and np.isfinite(float(lb))
    assert trg.global_step == step0 + 7


@pytest.mark.gpu
@pytest.mark.parametrize("fitted", [0, 1, 2, 3], ids=["random_init", "fitted_sphere", "half_the_rays_without_loss", "random_init_L24"])
def test_early_termination_leaves_every_gradient_bit_identical(fitted):
    """VERDICT r4 item 2 (north_star: "wavefront ballot/scan for ray compaction and early termination").  With the half-precision fused field the
    compositing backward writes exact zeros for rows whose gradients round to zero in the form k_field_bwd_x2 consumes them, reports the ray's dead
    32-row tiles by wave ballot, the field backward skips those tiles in place and the scatter emits no records for zero rows.  Skipped work adds
    exact zeros, so the table gradient (exact fixed-point sums) and the three MLP gradients (same tiles, same pipelines, same order) must be
    torch.equal to the run without it — on a random-initialised field (nothing to skip) and on a field fitted to the sphere scene (most of it);
    random_init_L24: a 24-level table, whose two-launch field backward evaluates every tile (the flushed rows are exact zeros there too)."""
    from customnerf_amd import scene as sc, tcnn, field as fld
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider_utils import generate_rays
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)
    H = W = 64
    V = 4
    torch.manual_seed(0)
    opt = sc.make_opt(fp16=True, num_steps=32, upsample_steps=32, iters=1000, num_levels=24 if fitted == 3 else 16)
    model = NeRFNetwork(opt).cuda()
    c2w = torch.from_numpy(sc.poses(V)).cuda()
    ro, rd = generate_rays(c2w, *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
    ro, rd = ro.view(V, 1, H * W, 3), rd.view(V, 1, H * W, 3)
    rgb, mask = sc.sphere_targets(ro.reshape(V, -1, 3), rd.reshape(V, -1, 3))
    kw = dict(num_steps=32, upsample_steps=32, dt_gamma=0, max_steps=1024)
    tr = ReconTrainer(model, opt, fp16=True)
    if fitted == 1:
        for i in range(200):
            tr.train_step(ro[i % V], rd[i % V], rgb[i % V], mask[i % V], **kw)
    g = torch.Generator(device="cuda").manual_seed(9)
    draws = dict(z=torch.rand(H * W, 32, device="cuda", generator=g), u=torch.rand(H * W, 32, device="cuda", generator=g))
    seen = []
    orig = fld.FieldFunction.backward

    def spy(ctx, g_sigma, g_rgbc):
        tl = getattr(g_sigma, '_cnerf_tile_live', None)
        tl = None if tl is None else tl[0]
        seen.append((None if tl is None else float(tl.float().mean()), float((g_sigma == 0).float().mean())))
        return orig(ctx, g_sigma, g_rgbc)
    fld.FieldFunction.backward = staticmethod(spy)
    try:
        grads = {}
        for et in (True, False):
            model.opt.early_termination = et
            for p in model.parameters():
                p.grad.zero_()
            model.train()
            with torch.autocast('cuda', dtype=torch.float16):
                out = model.render(ro[1], rd[1], staged=False, perturb=True, force_all_rays=True, _draws=draws, **kw)
                if fitted == 2:          # a loss that ignores the lower half of the image: those rays' gradients are exact zeros, their tiles dead
                    loss = (out['image'][:, :H * W // 2] ** 2).mean() + out['fg']['weights_sum'][:H * W // 2].mean()
                else:
                    loss = tr.loss(out, rgb[1], mask[1])
            tr.scaler.backward(loss)
            grads[et] = [p.grad.detach().clone() for p in model.parameters()]
    finally:
        fld.FieldFunction.backward = orig
        model.opt.early_termination = True
    (live_on, zero_on), (live_off, zero_off) = seen
    assert live_off is None and live_on is not None
    if fitted == 2:
        assert 0.45 < live_on < 0.55 and zero_on >= 0.5, seen                      # exactly the tiles of the rays that carry loss are live
    elif fitted == 1:
        assert zero_on > zero_off, seen                                             # rows flushed that were not exact zeros before
    else:
        assert live_on > 0.95, seen
    for a, b in zip(grads[True], grads[False]):
        assert torch.equal(a, b)
    assert all(bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 for a in grads[True])



@pytest.mark.gpu
def test_early_termination_flags_are_dropped_when_sigma_has_a_second_consumer():
    """the dead-tile flags ride on the gradient tensor the compositing backward hands to the field backward.  With a second
    differentiable consumer of sigma (a sparsity term) autograd ACCUMULATES into that tensor — in place, attribute and all — and stale flags
    would drop the second consumer's gradient for every 'dead' tile.  The hand-over carries address + version of both gradient tensors, so
    the flags are ignored here: the gradients must agree with the run without early termination (loosely: the flush itself rounds rows whose
    composite gradient is below half resolution to zero before the sum, which is below the tolerance; dropped tiles would not be)."""
    from customnerf_amd import scene as sc, tcnn, field as fld
    from customnerf_amd.nerf import render_ops
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider_utils import generate_rays
    from customnerf_amd.trainer import ReconTrainer
    tcnn.set_default_dtype(torch.float16)
    H = W = 64
    V = 4
    torch.manual_seed(0)
    opt = sc.make_opt(fp16=True, num_steps=32, upsample_steps=32, iters=1000)
    model = NeRFNetwork(opt).cuda()
    c2w = torch.from_numpy(sc.poses(V)).cuda()
    ro, rd = generate_rays(c2w, *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
    ro, rd = ro.view(V, 1, H * W, 3), rd.view(V, 1, H * W, 3)
    rgb, mask = sc.sphere_targets(ro.reshape(V, -1, 3), rd.reshape(V, -1, 3))
    kw = dict(num_steps=32, upsample_steps=32, dt_gamma=0, max_steps=1024)
    tr = ReconTrainer(model, opt, fp16=True)
    g = torch.Generator(device="cuda").manual_seed(9)
    draws = dict(z=torch.rand(H * W, 32, device="cuda", generator=g), u=torch.rand(H * W, 32, device="cuda", generator=g))
    captured, used = {}, []
    orig_c, orig_b = render_ops.composite_run_indexed, fld.FieldFunction.backward

    def tap(sig, rgbc, *a, **k):
        captured['sigma'], captured['rgbc'] = sig, rgbc
        return orig_c(sig, rgbc, *a, **k)

    def spy(ctx, g_sigma, g_rgbc):
        flags = getattr(g_sigma, '_cnerf_tile_live', None)
        ok = flags is not None and g_sigma.data_ptr() == flags[1] and g_sigma._version == flags[2] and g_rgbc.data_ptr() == flags[3] and g_rgbc._version == flags[4]
        used.append((flags is not None, ok, None if flags is None else float(flags[0].float().mean())))
        return orig_b(ctx, g_sigma, g_rgbc)
    render_ops.composite_run_indexed = tap
    fld.FieldFunction.backward = staticmethod(spy)
    try:
        grads = {}
        for second, et in ((True, True), (True, False), (False, True)):
            model.opt.early_termination = et
            for p in model.parameters():
                p.grad.zero_()
            model.train()
            with torch.autocast('cuda', dtype=torch.float16):
                out = model.render(ro[1], rd[1], staged=False, perturb=True, force_all_rays=True, _draws=draws, **kw)
                # a loss that ignores the lower half of the image: those rays' composite gradients are exact zeros, their tiles dead
                loss = (out['image'][:, :H * W // 2] ** 2).mean() + out['fg']['weights_sum'][:H * W // 2].mean()
            if second:                                       # second consumers of sigma AND of rgbc: every row gets gradient, dead tiles included
                loss = loss + 0.5 * captured['sigma'].float().mean() + 0.5 * captured['rgbc'].float().mean()
            tr.scaler.backward(loss)
            grads[(second, et)] = [p.grad.detach().clone() for p in model.parameters()]
    finally:
        render_ops.composite_run_indexed = orig_c
        fld.FieldFunction.backward = orig_b
        model.opt.early_termination = True
    (had1, ok1, live1), (had2, _, _), (had3, ok3, live3) = used
    assert not had2                                          # early termination off: no flags at all
    assert had3 and ok3 and 0.45 < live3 < 0.55              # single consumer: flags arrive intact, the tiles of the rays without loss are dead
    assert not ok1                                           # second consumer: whatever arrived no longer describes the tensors -> ignored
    for a, b in zip(grads[(True, True)], grads[(True, False)]):
        scale = float(b.abs().max())
        assert scale > 0 and float((a - b).abs().max()) <= 2e-3 * scale, (float((a - b).abs().max()), scale)
    # and the control: with stale flags the sparsity gradient of the dead tiles would be missing — it is a large part of these gradients
    diff = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(grads[(True, True)], grads[(False, True)]))
    assert diff > 1e-2, diff


@pytest.mark.gpu
def test_inf_check_is_folded_into_the_gradient_producers():
    """with the scaler watched (cnerf_scaler_watch) the field backward and the grid scatter raise found_inf themselves, and the
    trainer skips the pass over every gradient.  (1) the two producers raise the flag for a non-finite gradient — binned and atomic scatter sizes —
    and leave it alone otherwise; (2) a training step whose targets contain an infinity is skipped exactly as with the explicit check: parameters
    untouched, loss scale halved, gradients zeroed, the next clean step counts."""
    from customnerf_amd import tcnn
    from customnerf_amd.gridencoder import GridEncoder
    from customnerf_amd.optim import DynamicLossScaler
    tcnn.set_default_dtype(torch.float16)
    try:
        # (1) the scatter
        sclr = DynamicLossScaler(torch.device("cuda"))
        enc = GridEncoder(num_levels=16, log2_hashmap_size=19, desired_resolution=2048, gridtype='hash').cuda()
        for B in (70001, 3000):                                  # binned (>= 2^20 pairs) and atomic scatter
            x = torch.rand(B, 3, device="cuda") * 2 - 1
            for bad in (False, True):
                sclr.state[2] = 0.0
                enc.embeddings.grad = None
                out = enc.encode(x, bound=1.0, half=True)
                g = torch.randn_like(out) * 0.01
                if bad:
                    g[7, B // 2, 1] = float("inf")
                sclr.watch(True)
                try:
                    out.backward(g)
                finally:
                    sclr.watch(False)
                assert float(sclr.state[2]) == (1.0 if bad else 0.0), (B, bad)
                assert bool(torch.isfinite(enc.embeddings.grad).all()) == (not bad)
        # (2) the trainer
        _check_folded_inf_check_skips_a_step(16)
    finally:
        tcnn.set_default_dtype(torch.float32)


@pytest.mark.gpu
def test_inf_check_is_folded_into_the_gradient_producers_at_24_levels():
    """part (2) of the test above with a 24-level table: the field backward's two-launch form must raise found_inf itself"""
    from customnerf_amd import tcnn
    tcnn.set_default_dtype(torch.float16)
    try:
        _check_folded_inf_check_skips_a_step(24)
    finally:
        tcnn.set_default_dtype(torch.float32)


def _check_folded_inf_check_skips_a_step(num_levels):
    from customnerf_amd import scene as sc
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    H = W = 128
    o, d, rgb, mask = _target_scene(H, W, 2)
    results = {}
    for fold in (True, False):
        torch.manual_seed(0)
        opt = sc.make_opt(fp16=True, fold_inf_check=fold, num_levels=num_levels)
        model = NeRFNetwork(opt).cuda()
        tr = ReconTrainer(model, opt, fp16=True)
        kw = dict(num_steps=opt.num_steps, upsample_steps=opt.upsample_steps)
        tr.train_step(o[0], d[0], rgb[0], mask[0], **kw)
        assert tr._inf_folded == fold
        before = [p.detach().clone() for p in model.parameters()]
        bad_rgb = rgb[1].clone()
        bad_rgb[1234, 1] = float("inf")
        loss, _ = tr.train_step(o[1], d[1], bad_rgb, mask[1], **kw)
        st = tr.scaler.state.detach().cpu().tolist()
        assert not np.isfinite(float(loss))
        assert st[0] == 32768.0 and st[2] == 0.0 and st[3] == 1.0, st           # backed off, flag cleared, still one good step
        for a, p in zip(before, model.parameters()):
            assert torch.equal(a, p.detach())                                      # the optimiser step was skipped
            assert bool((p.grad == 0).all())                                       # ... and the gradients were zeroed all the same
        loss, _ = tr.train_step(o[0], d[0], rgb[0], mask[0], **kw)
        assert np.isfinite(float(loss)) and tr.scaler.good_steps() == 2
        results[fold] = [p.detach().clone() for p in model.parameters()]
    for a, b in zip(results[True], results[False]):
        assert torch.equal(a, b)                                                   # the folded check changes no bit of the training
