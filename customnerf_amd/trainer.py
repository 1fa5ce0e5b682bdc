"""Minimal counterpart of the reference trainer's reconstruction step (nerf/utils_init_nerf.py:194-241
`train_step_pretrain`, :599-629 the loop body) with the reference's optimiser recipe (main.py:182-189) and the
data-parallel layer the reference lacks: ray/view sharding across ranks, one RCCL all-reduce of
the flattened gradients per step.
"""
import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _coll
from .optim import DynamicLossScaler, FusedAdam


def flat_grad_buffer(parameters):
    """Give every trainable parameter a persistent, zeroed `.grad` that is a view into ONE flat fp32 buffer (parameter order), so that
    the per-step all-reduce runs in place on that buffer: no gather / scatter copies around the collective.  autograd accumulates into an
    existing `.grad` in place and the fused Adam step zeroes it in place, so the views stay bound."""
    ps = [p for p in parameters if p.requires_grad]
    if not ps:
        return None
    flat = torch.zeros(sum(_slot(p.numel()) for p in ps), dtype=torch.float32, device=ps[0].device)
    off = 0
    for p in ps:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += _slot(p.numel())
    return flat


def enable_grad_in_place(model):
    """With persistent .grad views (flat_grad_buffer) the grid scatter may add straight into embeddings.grad (GridEncoder.grad_in_place):
    autograd then has nothing to accumulate for the table."""
    enc = getattr(model, 'pos_en', None)
    if enc is not None and hasattr(enc, 'attach_backward'):
        enc.grad_in_place = True
    model.grad_in_place = True                          # the fused field's three parameter vectors (NeRFNetwork.split_forward)


def _slot(n):
    return (n + 3) // 4 * 4            # every view starts 16-byte aligned (the fused Adam kernel loads float4); pad elements stay zero


def _grads_alias_flat(grads, flat):
    off = flat.data_ptr()
    for g in grads:
        if g.dtype != flat.dtype or not g.is_contiguous() or g.data_ptr() != off:
            return False
        off += _slot(g.numel()) * flat.element_size()
    return off == flat.data_ptr() + flat.numel() * flat.element_size()


def allreduce_grads_flat(parameters, flat, world_size):
    """One flattened all-reduce (sum) of all gradients (RCCL over xGMI on GPUs, gloo in the CPU tests); returns the flat buffer
    for reuse.  In place when the gradients are views of `flat` (flat_grad_buffer), through a staging copy otherwise.  The 1/world
    factor is NOT applied here (folded into the Adam un-scale).  Shared by ReconTrainer and EditTrainer."""
    if world_size <= 1:
        return flat
    grads = [p.grad for p in parameters if p.grad is not None]
    if flat is not None and _grads_alias_flat(grads, flat):
        _coll.all_reduce(flat, op=dist.ReduceOp.SUM)
        return flat
    n = sum(g.numel() for g in grads)
    if flat is None or flat.numel() != n:
        flat = torch.empty(n, dtype=torch.float32, device=grads[0].device)       # staging buffer (the caller keeps it for the next step)
    torch._foreach_copy_(list(flat.split([g.numel() for g in grads])), [g.reshape(-1) for g in grads])
    _coll.all_reduce(flat, op=dist.ReduceOp.SUM)
    torch._foreach_copy_([g.reshape(-1) for g in grads], list(flat.split([g.numel() for g in grads])))
    return flat


def register_half_shadow(optimizer, model, fp16):
    """Let the fused Adam refresh the grid table's fp16 shadow in its own pass (no separate cast launch per step)."""
    enc = getattr(model, 'pos_en', None)
    if fp16 and enc is not None and hasattr(enc, 'half_table') and enc.embeddings.is_cuda and enc.level_dim % 2 == 0:
        optimizer.half_shadows[enc.embeddings] = enc.half_table()


def refresh_half_shadow(optimizer, model):
    enc = getattr(model, 'pos_en', None)
    if enc is not None and enc.embeddings in optimizer.half_shadows:
        enc.set_half_table(optimizer.half_shadows[enc.embeddings])   # the step just rewrote it: mark it current


class packed_weights_window:
    """`with packed_weights_window(model):` — for the duration of a training step the fused field kernels read the packed fp16 image of the MLP
    parameters (NeRFNetwork._weight_image / field.packed_weights: one pack launch per parameter version instead of 14 us of staging in each
    of the step's three field launches).  Only inside the step: there every parameter write goes through the trainer's optimiser, which moves
    the version counters the image is keyed on; outside (evaluation under torch_ema's `.data` swaps, user code) the kernels stage from the
    float32 parameters.  `opt.packed_field_weights = False` switches it off."""

    def __init__(self, model, opt=None):
        self.d = getattr(model, '__dict__', None) if getattr(opt, 'packed_field_weights', True) else None

    def __enter__(self):
        if self.d is not None:
            self.prev = self.d.get('packed_field_weights', False)
            self.d['packed_field_weights'] = True

    def __exit__(self, *exc):
        if self.d is not None:
            self.d['packed_field_weights'] = self.prev
        return False


def ray_reg_wanted(opt):
    """do the options ask for a regulariser of the ray weights (opt.lambda_distortion / opt.lambda_ray_entropy, both 0 by default)?  The trainers
    pass ray_reg=True to the renderer only then: without it no launch is added and the result dict keeps its keys."""
    return bool(getattr(opt, 'lambda_distortion', 0) or getattr(opt, 'lambda_ray_entropy', 0))


def ray_reg_loss(opt, outputs):
    """lambda_distortion * mean over rays of outputs['distortion'] + lambda_ray_entropy * mean of outputs['ray_entropy'] (run(ray_reg=True); pass
    the result dict, or its 'fg' / 'bg' entry) -> (sum, {'loss_distortion': ..., 'loss_ray_entropy': ...} with the weighted terms, detached)"""
    total, terms = 0.0, {}
    for lam, key, name in ((getattr(opt, 'lambda_distortion', 0), 'distortion', 'loss_distortion'),
                           (getattr(opt, 'lambda_ray_entropy', 0), 'ray_entropy', 'loss_ray_entropy')):
        if lam:
            term = float(lam) * outputs[key].float().mean()
            total = total + term
            terms[name] = term.detach()
    return total, terms


def dssim_wanted(opt):
    """do the options ask for the structural image term (opt.lambda_dssim, absent or 0 by default)?  Without it the step adds no launch."""
    return bool(getattr(opt, 'lambda_dssim', 0))


def dssim_check(opt, image_hw, n_rays, select_inds=None):
    """The D-SSIM term reads the step's rays as ONE whole H x W view, row-major: with opt.lambda_dssim set, image_hw = (H, W) is required,
    H W is the number of rays, nothing subsamples them and both extents hold a window.  ValueError otherwise, before anything is rendered."""
    if not dssim_wanted(opt):
        return
    if image_hw is None:
        raise ValueError("lambda_dssim: pass image_hw=(H, W), the extents of the view the rays cover")
    try:
        H, W = (int(v) for v in image_hw)
    except (TypeError, ValueError):
        raise ValueError(f"lambda_dssim: image_hw must be (H, W), got {image_hw!r}") from None
    if int(getattr(opt, 'batch_rays', 0) or 0) > 0 or select_inds is not None:
        raise ValueError("lambda_dssim: the term needs the whole view, not a batch_rays subset of its rays")
    if H * W != n_rays:
        raise ValueError(f"lambda_dssim: image_hw {H} x {W} does not cover the step's {n_rays} rays")
    if H < 11 or W < 11:
        raise ValueError(f"lambda_dssim: a view of {H} x {W} is smaller than one 11 x 11 SSIM window")


def dssim_loss(opt, outputs, rgbs, image_hw):
    """lambda_dssim * (1 - SSIM(outputs['image'], rgbs)) on the view as one [1, H, W, 3] image (metrics.ssim_loss: the 3D-Gaussian-splatting
    recipe's structural term; the gradient goes to the prediction only)"""
    from .metrics import ssim_loss
    if image_hw is None:
        raise ValueError("lambda_dssim: pass image_hw=(H, W), the extents of the view the rays cover")
    H, W = (int(v) for v in image_hw)
    image = outputs['image'].reshape(1, H, W, 3).float()
    return float(opt.lambda_dssim) * ssim_loss(image, rgbs.reshape(1, H, W, 3).to(image.dtype))


def inf_check_is_folded(trainer):
    """Round 6: GradScaler's inf check is a pass over every gradient (9 us for the benchmark table, 30 us for the reference
    field's).  With the scaler WATCHED (DynamicLossScaler.watch) the two kernels that produce the gradients raise found_inf themselves — the field
    backward's partial reduction for the three MLPs, the scatter's emit for the table (a non-finite incoming gradient is the only way its exact
    fixed-point sums can go non-finite) — so the pass is skipped when EVERY trainable parameter is one of those four tensors of a fused
    half-precision NeRFNetwork and no gradient exchange runs in between (the exchange checks its own reduced shards)."""
    m = trainer.model
    if trainer.world_size != 1 or getattr(trainer, '_dp', None) is not None or trainer.scaler is None or not getattr(trainer, 'fused_adam', True):
        return False
    if not (hasattr(m, '_fused_cfg') and hasattr(m, '_half') and hasattr(m, 'pos_en') and getattr(m, 'grad_in_place', False)):
        return False
    try:
        if not (m._fused_cfg() and m._half()):
            return False
        known = {id(m.pos_en.embeddings), id(m.network.params), id(m.density_network.params), id(m.rgb_network.params)}
    except Exception:
        return False
    return all(id(p) in known for p in m.parameters() if p.requires_grad) and bool(getattr(trainer.opt, 'fold_inf_check', True))


def check_grads_finite(scaler, parameters, flat):
    """GradScaler's inf check on the (all-reduced) gradients: one pass over the flat buffer when the gradients alias it."""
    grads = [p.grad for p in parameters if p.grad is not None]
    if flat is not None and _grads_alias_flat(grads, flat):
        scaler.check(flat)
    else:
        for g in grads:
            scaler.check(g.contiguous())


def setup_sharded_dp(trainer, model, fp16, rank=None, group=None):
    """dp_mode 'sharded' (customnerf_amd.dp.ShardedExchange): the big parameters (the grid table) leave the trainer's FusedAdam — their owner
    shards are updated by the exchange (and, only with `dp.async_ops`, the MLP all-reduce is hooked in front of the grid scatter)."""
    from .dp import ShardedExchange, BIG_PARAM_MIN
    opt_ = trainer.optimizer
    lr_by_id = {id(p): i for i, g in enumerate(opt_.param_groups) for p in g['params']}
    params = [p for p in model.parameters() if p.requires_grad]
    enc = getattr(model, 'pos_en', None)
    half = bool(fp16 and enc is not None and hasattr(enc, 'half_table') and enc.level_dim % 2 == 0)
    rank = dist.get_rank(group) if rank is None else rank
    dp = ShardedExchange(params, trainer._flat, lambda p: trainer.base_lrs[lr_by_id[id(p)]], trainer.world_size, rank, betas=(0.9, 0.99), eps=1e-15,
                         scaler=trainer.scaler, half_shadow=half, group=group)
    opt_.skip_params = {id(st['p']) for st in dp.state}
    if half and enc is not None:
        sh = dp.shadow_table(enc.embeddings)
        if sh is not None:
            opt_.half_shadows[enc.embeddings] = sh                 # refresh_half_shadow hands it to the encoder after every step
            enc.set_half_table(sh)
    if dp.async_ops and enc is not None and hasattr(enc, 'attach_backward'):
        from .gridencoder import grid as ge
        ge.set_pre_scatter_hook(dp.start_small)                    # MLP gradients go out while the grid scatter still runs
    return dp


def apply_optimizer_step(trainer):
    """gradient exchange + GradScaler check + Adam + scaler update + fp16 shadow hand-over, for ReconTrainer and EditTrainer (fused Adam path).
    world_size 1: no exchange; dp_mode 'allreduce': one in-place fp32 all-reduce of the flat buffer; 'sharded': dp.ShardedExchange."""
    f = trainer.lr_factor()
    for g, base in zip(trainer.optimizer.param_groups, trainer.base_lrs):
        g['lr'] = base * f
    dp = getattr(trainer, '_dp', None)
    trainer.optimizer.grad_scale_inv = 1.0 / (trainer.loss_scale * trainer.world_size)
    if dp is not None:
        ev = getattr(trainer, '_exchange_events', None)              # bench.py: event pairs around the exchange (None = off)
        if ev is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        dp.exchange()
        dp.check()
        dp.step(f, trainer.loss_scale)
        if ev is not None:
            e1.record()
            ev.append((e0, e1))
        trainer.optimizer.step()                                     # the small (replicated) parameters; the big ones are in skip_params
        if trainer.scaler is not None:
            trainer.scaler.update()                                  # (a no-op when FusedAdam's multi-tensor launch of the small tensors already did it)
    else:
        trainer.allreduce_grads()
        if trainer.scaler is not None:
            if not getattr(trainer, '_inf_folded', False):
                check_grads_finite(trainer.scaler, list(trainer.model.parameters()), trainer._flat)  # on the all-reduced gradients: every rank takes the same skip decision
            trainer.optimizer.step()
            trainer.scaler.update()                                  # (a no-op when FusedAdam's multi-tensor launch of the small tensors already did it)
        else:
            trainer.optimizer.step()
    refresh_half_shadow(trainer.optimizer, trainer.model)


class CheckpointMixin:
    """Checkpoints of a (possibly sharded data-parallel) trainer.  In dp_mode 'sharded' with the fp16 shadow the optimiser updates the owners'
    float32 master SHARDS and the shadow table only; the float32 nn.Parameter is refreshed here (ShardedExchange.consolidate — a collective, so
    EVERY rank calls these methods; rank 0 writes the file).  checkpoint.checkpoint_state refuses a model whose parameters are marked stale."""

    def state_dict(self):
        if getattr(self, '_dp', None) is not None:
            self._dp.consolidate()
        return self.model.state_dict()

    def save_checkpoint(self, path, epoch=0, stats=None, full=False, rank=None):
        from . import checkpoint
        dp = getattr(self, '_dp', None)
        if dp is not None:
            if full:
                dp.export_optimizer_state(self.optimizer)         # consolidates + gathers the sharded Adam moments into the unsharded layout
            else:
                dp.consolidate()
        if rank is None:
            rank = dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0
        if rank != 0:
            return None
        return checkpoint.save_checkpoint(path, self.model, epoch=epoch, global_step=self.global_step, stats=stats, optimizer=self.optimizer, full=full,
                                          scaler=self.scaler)

    def _graph_inputs(self):
        """addresses of everything a captured step (train_step_graphed) reads or writes that a load could move: the parameters, their persistent
        gradients, the model's buffers, the fp16 shadow of the grid table, the loss scaler's state"""
        enc = getattr(self.model, 'pos_en', None)
        shadow = getattr(enc, '_half_table', None)
        ts = [t for p in self.model.parameters() for t in (p, p.grad)] + list(self.model.buffers()) + [shadow, getattr(self.scaler, 'state', None)]
        return [None if t is None else (t.data_ptr(), t.dtype, tuple(t.shape)) for t in ts]

    def load_checkpoint(self, path_or_dict, model_only=False):
        """Counterpart of save_checkpoint (checkpoint.load_checkpoint with this trainer's optimiser and loss scaler; Trainer_Nerf.load_checkpoint,
        utils_init_nerf.py:837-901) for a fresh trainer and for rolling a live one back.  -> checkpoint.load_checkpoint's info dict.
        The parameter values are copied IN PLACE (the flat gradient buffer, the fp16 shadow and captured graphs are bound to the parameter storage);
        `global_step` — which the learning-rate decay is a function of — is restored (and `epoch` / `stats` on a trainer that keeps them); the Adam
        moments are new tensors afterwards, so an armed table step is dropped; in dp_mode 'sharded' the shards are re-cut from the loaded tensors
        (every rank calls this).  Captured graphs survive unless something they reference moved."""
        from . import checkpoint
        opt_ = self.optimizer
        if hasattr(opt_, 'disarm_in_backward'):
            opt_.disarm_in_backward()                                 # (FusedAdam.load_state_dict does it too; a model_only load never gets there)
        before = self._graph_inputs()
        dev = next(self.model.parameters()).device
        info = checkpoint.load_checkpoint(self.model, path_or_dict, model_only=model_only, optimizer=opt_, scaler=self.scaler, map_location=dev)
        if not model_only:
            if info['global_step'] is not None:
                self.global_step = int(info['global_step'])
            for k in ('epoch', 'stats'):
                if hasattr(self, k) and info[k] is not None:
                    setattr(self, k, info[k])
        enc = getattr(self.model, 'pos_en', None)
        dp = getattr(self, '_dp', None)
        if dp is not None:
            dp.import_optimizer_state(opt_, moments=not model_only)  # master shards, sharded moments and the shadow table from the loaded tensors
            refresh_half_shadow(opt_, self.model)
        else:
            sh = getattr(opt_, 'half_shadows', {}).get(enc.embeddings) if enc is not None else None
            if sh is not None:
                # the shadow the fused Adam step writes IS the encoder's: re-cast it now from the loaded table
                enc.set_half_table(sh)
                enc.invalidate_half_table()
                enc.half_table()
        if self._graph_inputs() != before:
            self.__dict__.pop('_graphs', None)
            self.__dict__.pop('_graph_pool', None)
            self.__dict__.pop('_graph_gen', None)
        return info


class EvalMixin:
    """Trainer_Nerf.eval_step / test_step (nerf/utils_init_nerf.py:396-434, 436-485): one full view rendered without perturbation and the image
    panels the reference's evaluate_one_epoch / test loops write out.  The reference passes `**vars(self.opt)` to render(); the sampling keys
    run() / run_cuda() read are forwarded here.  (Its render() ignores `staged` — renderer.py:1719-1733 — as this package's does.)"""

    def _render_eval(self, model, rays_o, rays_d, perturb=False):
        opt = self.opt
        kw = dict(num_steps=opt.num_steps, upsample_steps=opt.upsample_steps, dt_gamma=getattr(opt, 'dt_gamma', 0), max_steps=opt.max_steps)
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16, enabled=self.fp16):
            return model.render(rays_o, rays_d, staged=True, perturb=perturb, force_all_rays=True, **kw)

    def eval_step(self, data):
        """-> (panel [B, H, n W, 3] = gt | prediction | depth (| gt mask | predicted mask | foreground | background under opt.train_conf), None, None,
        loss = tensor([0])), as utils_init_nerf.py:396-434"""
        rgbs, mask, rays_o, rays_d, H, W, _ = data
        dev = next(self.model.parameters()).device
        rgbs, mask, rays_o, rays_d = rgbs.to(dev), mask.to(dev), rays_o.to(dev), rays_d.to(dev)
        B = rays_o.shape[0]
        outputs = self._render_eval(self.model, rays_o, rays_d)
        ims = [rgbs.reshape(B, H, W, 3).float(), outputs['image'].reshape(B, H, W, 3).float(), outputs['depth'].reshape(B, H, W, 1).float().repeat(1, 1, 1, 3)]
        if getattr(self.opt, 'train_conf', 0):
            ims += [mask.reshape(B, H, W, 1).float().repeat(1, 1, 1, 3),
                    outputs['render_mask'].reshape(B, H, W, -1).float().mean(-1, keepdim=True).repeat(1, 1, 1, 3),
                    outputs['fg']['image'].reshape(B, H, W, 3).float(), outputs['bg']['image'].reshape(B, H, W, 3).float()]
        return torch.cat(ims, dim=2), None, None, torch.tensor([0])

    def test_step(self, data, bg_color=None, perturb=False, if_gui=False):
        """-> (pred_rgb [B, H, W, 3] — the panel prediction | mask | foreground | background under opt.train_conf and opt.render_all —,
        pred_depth [B, H, W], dir), as utils_init_nerf.py:436-485.  (The reference also renders model_pretrained there and drops the result.)"""
        direction = torch.tensor(0)
        if if_gui:
            rays_o, rays_d, H, W, direction = data['rays_o'], data['rays_d'], data['H'], data['W'], data['dir']
        else:
            _, _, rays_o, rays_d, H, W, _ = data
        dev = next(self.model.parameters()).device
        rays_o, rays_d = rays_o.to(dev), rays_d.to(dev)
        B = rays_o.shape[0]
        outputs = self._render_eval(self.model, rays_o, rays_d, perturb=perturb)
        pred_rgb = outputs['image'].reshape(B, H, W, 3).float()
        pred_depth = outputs['depth'].reshape(B, H, W).float()
        if getattr(self.opt, 'train_conf', 0) and getattr(self.opt, 'render_all', False):
            pred_rgb = torch.cat([pred_rgb, outputs['render_mask'].reshape(B, H, W, 1).float().repeat(1, 1, 1, 3),
                                  outputs['fg']['image'].reshape(B, H, W, 3).float(), outputs['bg']['image'].reshape(B, H, W, 3).float()], dim=2)
        return pred_rgb, pred_depth, direction

    class _eval_mode:
        """`with self._eval_mode(models):` — model.eval() for the duration of a loop (Trainer_Nerf.evaluate_one_epoch / test do the same and
        never switch back; here whatever mode each model was in is restored)"""

        def __init__(self, *models):
            self.models = [m for m in models if m is not None]

        def __enter__(self):
            self.was = [m.training for m in self.models]
            for m in self.models:
                m.eval()

        def __exit__(self, *exc):
            for m, w in zip(self.models, self.was):
                m.train(w)
            return False

    def evaluate(self, views, save_path=None, name=None, quantize=False, against=None):
        """The loop around eval_step (Trainer_Nerf.evaluate / evaluate_one_epoch, utils_init_nerf.py:515-518, :673-779) with the scores the
        reference never computes.  views: an indexable of view tuples (rgbs, mask, rays_o, rays_d, H, W, path) WITH images — a
        NerfstudioScene of split 'val', say.  Per view: eval_step, then metrics.image_metrics(prediction, ground truth) -> 'mse', 'l1',
        'psnr', 'ssim' (metrics.py defines them; quantize=True scores what 8-bit files of the two images hold); where the view has a mask
        (not None), the same four over the masked foreground, 'fg_*', and over the rest (1 - mask), 'bg_*', with the counted pixel-channels
        'fg_n_pixels' / 'bg_n_pixels'; under opt.train_conf 'mask_iou', the intersection over union of render_mask > 0.5 and the mask.

        against=<another field> is the background-preservation report of an edit instead: nothing is compared with the photographs; both
        `against` (the pretrained field) and self.model render the view's rays and the scores are between those two renders, so 'bg_psnr' /
        'bg_ssim' say how well the edit left alone what it was told to leave alone (views without images will do, a mask is needed for the
        fg / bg part).

        -> {'views': [one dict of floats per view], 'mean': {key: mean over the views, nan entries — an empty mask — left out}}.
        save_path: the panels (eval_step's, or `against | edited`) are written as <save_path>/<name>/<i:04d>.png (mesh.write_png,
        floor(clamp(v, 0, 1) * 255)) and the returned dict as metrics.json beside them; name defaults to 'evaluate'."""
        import json
        import os
        from . import metrics as M
        from .mesh import write_png
        name = name or 'evaluate'
        if save_path is not None:
            os.makedirs(os.path.join(save_path, name), exist_ok=True)
        dev = next(self.model.parameters()).device
        rows = []
        with self._eval_mode(self.model, against):
            for i in range(len(views)):
                data = views[i]
                rgbs, mask, rays_o, rays_d, H, W = data[:6]
                row = {}
                if against is None:
                    if rgbs is None or mask is None:
                        raise ValueError("evaluate: the views need images and masks (a 'val' or 'train' split), or pass against=")
                    panel = self.eval_step(data)[0]
                    ref, pred = panel[:, :, :W].contiguous(), panel[:, :, W:2 * W].contiguous()
                    if getattr(self.opt, 'train_conf', 0):
                        gt_m, pr_m = panel[:, :, 3 * W:4 * W, 0] > 0.5, panel[:, :, 4 * W:5 * W, 0] > 0.5
                        union = (gt_m | pr_m).sum()
                        row['mask_iou'] = (gt_m & pr_m).sum().double() / union.double()          # nan when both are empty
                else:
                    rays_o, rays_d = rays_o.to(dev), rays_d.to(dev)
                    B = rays_o.shape[0]
                    ref = self._render_eval(against, rays_o, rays_d)['image'].reshape(B, H, W, 3).float()
                    pred = self._render_eval(self.model, rays_o, rays_d)['image'].reshape(B, H, W, 3).float()
                    panel = torch.cat([ref, pred], dim=2)
                regions = [('', None)]
                if mask is not None:
                    fg = (mask.to(dev).reshape(pred.shape[0], H, W) != 0).float()
                    regions += [('fg_', fg), ('bg_', 1.0 - fg)]
                for prefix, m in regions:
                    r = M.image_metrics(pred, ref, mask=m, quantize=quantize)
                    for k in ('mse', 'l1', 'psnr', 'ssim') + (('n_pixels',) if prefix else ()):
                        row[prefix + k] = r[k].mean() if k != 'n_pixels' else r[k].sum()
                rows.append(row)
                if save_path is not None:
                    write_png(os.path.join(save_path, name, f'{i:04d}.png'), M.to_uint8(panel[0]))
        rows = [{k: float(v) for k, v in row.items()} for row in rows]                          # the host reads the scores only after the loop
        mean = {}
        for k in (rows[0] if rows else {}):
            vals = [r[k] for r in rows if k in r and r[k] == r[k]]
            mean[k] = sum(vals) / len(vals) if vals else float('nan')
        out = {'views': rows, 'mean': mean}
        if save_path is not None:
            with open(os.path.join(save_path, name, 'metrics.json'), 'w') as fh:
                json.dump(out, fh, indent=1)                                                    # (inf / nan as Python's json writes and reads them)
        return out

    def test(self, views, save_path, name=None, write_video=True, fps=30):
        """The loop around test_step (Trainer_Nerf.test, utils_init_nerf.py:520-569): every view of `views` (a NerfstudioScene of split 'test',
        say; images are not needed) is rendered and written as <save_path>/<name>/<i:03d>.png by the reference's truncation
        floor(clamp(v, 0, 1) * 255) (:550; metrics.to_uint8 — what image_metrics(quantize=True) scores).  write_video: all frames also go
        into ONE animated PNG, <save_path>/<name>_rgb.png, `fps` frames a second (mesh.write_apng).  The reference writes an MP4 through
        imageio there; no MP4 encoder is part of this package, and an APNG is the one-file substitute that browsers open.
        -> {'frames': [paths], 'video': path or None}.  name defaults to 'test'."""
        import os
        from . import metrics as M
        from .mesh import write_apng, write_png
        name = name or 'test'
        os.makedirs(os.path.join(save_path, name), exist_ok=True)
        frames, paths = [], []
        with self._eval_mode(self.model):
            for i in range(len(views)):
                pred = self.test_step(views[i])[0]
                frame = M.to_uint8(pred[0]).cpu()
                paths.append(os.path.join(save_path, name, f'{i:03d}.png'))
                write_png(paths[-1], frame)
                if write_video:
                    frames.append(frame)
        video = None
        if write_video and frames:
            video = os.path.join(save_path, f'{name}_rgb.png')
            write_apng(video, frames, fps=fps)
        return {'frames': paths, 'video': video}


class ReconTrainer(CheckpointMixin, EvalMixin):
    def __init__(self, model, opt, lr=None, fp16=False, world_size=1, fused_adam=True, loss_scale='dynamic', dp_mode='allreduce'):
        """dp_mode (world_size > 1): 'allreduce' = one in-place fp32 all-reduce of the flat gradient buffer; 'sharded' = customnerf_amd.dp.ShardedExchange
        (fp16 all-to-all payload summed in fp32 on arrival, sharded Adam, all-gather of the fp16 shadow; MLP groups all-reduced in fp32).
        loss_scale: 'dynamic' = the reference's GradScaler policy (utils_init_nerf.py `self.scaler = GradScaler(enabled=self.fp16)`:
        init 65536, x2 / 2000 clean steps, x0.5 + skipped step on inf) kept on the device (optim.DynamicLossScaler, fused Adam only);
        a float = static scale."""
        self.model, self.opt = model, opt
        self.fp16 = fp16
        self.world_size = world_size
        self.dp_mode = dp_mode if world_size > 1 else 'none'
        if loss_scale == 'dynamic' and not (fp16 and fused_adam):
            loss_scale = 128.0
        self.scaler = DynamicLossScaler(next(model.parameters()).device) if loss_scale == 'dynamic' else None
        self.loss_scale = 1.0 if (not fp16 or self.scaler is not None) else float(loss_scale)
        lr = opt.lr if lr is None else lr
        groups = model.get_params(lr)                        # grid lr x10 (network_grid.py:196-206)
        self.base_lrs = [g['lr'] for g in groups]
        if fused_adam:
            self.optimizer = FusedAdam(groups, betas=(0.9, 0.99), eps=1e-15)
            self.optimizer.scaler = self.scaler
            register_half_shadow(self.optimizer, model, fp16)
        else:
            self.optimizer = torch.optim.Adam(groups, betas=(0.9, 0.99), eps=1e-15)
        self.fused_adam = fused_adam
        self.global_step = 0
        self._flat = flat_grad_buffer(self.model.parameters())   # persistent, pre-zeroed .grad views of one flat buffer (zeroed by the fused step)
        if fused_adam:
            enable_grad_in_place(model)                          # (torch.optim.Adam + zero_grad keeps the views too, but stay on the plain path there)
        self._dp = setup_sharded_dp(self, model, fp16) if (self.dp_mode == 'sharded' and fused_adam) else None

    def lr_factor(self):
        return 0.1 ** min(self.global_step / self.opt.iters, 1)      # main.py:189

    def dp_describe(self):
        """one-line description of the gradient exchange (bench.py's config.parallelism)"""
        if self.dp_mode == 'sharded' and getattr(self, '_dp', None) is not None:
            return self._dp.describe()
        return "fp32 grad all-reduce, in place on the flat buffer"

    def loss(self, outputs, rgbs, mask, image_hw=None):
        """utils_init_nerf.py:220-234, plus the regularisers of the ray weights (`all` composite) where opt.lambda_distortion /
        opt.lambda_ray_entropy ask for them, plus opt.lambda_dssim * (1 - SSIM) of the view (image_hw = (H, W), row-major rays) where
        that is set.  outputs['image'] is a view of the composite output the fused loss reads: autograd adds the two gradients before
        the one compositing backward."""
        loss = ReconTrainer.recon_loss(self, outputs, rgbs, mask)               # (callers may pass any object with `opt` as self)
        if ray_reg_wanted(self.opt):
            loss = loss + ray_reg_loss(self.opt, outputs)[0]
        if dssim_wanted(self.opt):
            loss = loss + dssim_loss(self.opt, outputs, rgbs, image_hw)
        return loss

    def recon_loss(self, outputs, rgbs, mask):
        """utils_init_nerf.py:220-234"""
        if '_out_ray' in outputs and outputs['_out_ray'].is_cuda and getattr(self.opt, 'fused_loss', True):
            from .nerf.render_ops import recon_loss                   # loss + gradient in one launch on the fused renderer's composite output
            with_mask = bool(getattr(self.opt, 'train_conf', 0)) and 'render_mask' in outputs
            sc = getattr(self, 'scaler', None)                        # the backward seed (DynamicLossScaler.backward) folded into the loss gradient
            return recon_loss(outputs['_out_ray'], rgbs, mask if with_mask else None, getattr(self.opt, 'train_rgb', 1.0),
                              getattr(self.opt, 'train_conf', 0) if with_mask else 0.0, sc.state[0:1] if sc is not None else None)
        pred_rgb = outputs['image']
        loss = getattr(self.opt, 'train_rgb', 1.0) * F.mse_loss(pred_rgb.reshape(-1, 3).float(), rgbs.reshape(-1, 3))
        if getattr(self.opt, 'train_conf', 0) and 'render_mask' in outputs:
            loss = loss + self.opt.train_conf * F.mse_loss(outputs['render_mask'].reshape(-1).float(), mask.reshape(-1))
        return loss

    def allreduce_grads(self):
        """One flattened RCCL all-reduce (sum) per step; the 1/world factor is folded into the Adam un-scale."""
        self._flat = allreduce_grads_flat(list(self.model.parameters()), self._flat, self.world_size)

    def select_rays(self, rays_o, rays_d, rgbs, mask, select_inds=None):
        """`--batch_rays` (utils_init_nerf.py:210-215): a random subset of `opt.batch_rays` rays of the view, drawn without replacement by
        numpy on the host as the reference does (`np.random.choice`; `select_inds` replays a recorded draw), gathered on the device."""
        n = int(getattr(self.opt, 'batch_rays', 0) or 0)
        if not n and select_inds is None:
            return rays_o, rays_d, rgbs, mask
        N = rays_o.reshape(-1, 3).shape[0]
        if select_inds is None:
            import numpy as np
            select_inds = np.random.choice(N, size=[n], replace=False)
        idx = torch.as_tensor(select_inds, dtype=torch.long).to(rays_o.device)
        pick = lambda t, c: t.reshape(1, N, c).index_select(1, idx) if t is not None else None
        return pick(rays_o, 3), pick(rays_d, 3), pick(rgbs, 3), pick(mask, 1)

    def _watch_scaler(self):
        """at the start of every step: is the inf check folded into the gradient producers (inf_check_is_folded), and if so point them at this scaler"""
        self._inf_folded = inf_check_is_folded(self)
        if self.scaler is not None:
            self.scaler.watch(self._inf_folded)

    def train_step(self, rays_o, rays_d, rgbs, mask, select_inds=None, **render_kw):
        self._watch_scaler()
        try:
            with packed_weights_window(self.model, self.opt):
                return self._train_step(rays_o, rays_d, rgbs, mask, select_inds, **render_kw)
        finally:
            if self.scaler is not None:
                self.scaler.watch(False)                 # (the library holds a raw pointer into the scaler's state only for the duration of a step)

    def _arm_table_step(self):
        """The grid table's Adam update inside the backward scatter (optim.FusedAdam.arm_in_backward): only where this step's ONE backward pass is the
        table gradient's only source and found_inf is final when the scatter runs — fused Adam with the on-device scaler, the inf check folded into
        the field's gradient producers (inf_check_is_folded: every trainable parameter is the fused field's, persistent in-place gradients), one
        GPU, eager (a captured backward would freeze the learning rate).  `opt.fuse_table_adam = False` switches it off."""
        if not (self.fused_adam and getattr(self, '_inf_folded', False) and self.world_size == 1 and getattr(self, '_dp', None) is None
                and getattr(self.opt, 'fuse_table_adam', True) and not torch.cuda.is_current_stream_capturing()):
            return False
        f = self.lr_factor()                                          # (apply_optimizer_step sets the same values again after the backward pass)
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g['lr'] = base * f
        self.optimizer.grad_scale_inv = 1.0 / (self.loss_scale * self.world_size)
        return self.optimizer.arm_in_backward(self.model.pos_en.embeddings)

    def _train_step(self, rays_o, rays_d, rgbs, mask, select_inds=None, **render_kw):
        image_hw = render_kw.pop('image_hw', None)                               # (H, W) of the view: the D-SSIM term's, not the renderer's
        dssim_check(self.opt, image_hw, rays_o.reshape(-1, 3).shape[0], select_inds)
        self.model.train()
        rays_o, rays_d, rgbs, mask = self.select_rays(rays_o, rays_d, rgbs, mask, select_inds)
        render_kw.setdefault('fg_bg', getattr(self, 'needs_fg_bg', False))       # the reconstruction loss reads the first composite only
        if ray_reg_wanted(self.opt):
            render_kw.setdefault('ray_reg', True)
        with torch.autocast('cuda', dtype=torch.float16, enabled=self.fp16):
            outputs = self.model.render(rays_o, rays_d, staged=False, perturb=True, force_all_rays=True, **render_kw)
            # (image_hw only where the term is on: a subclass's three-argument loss() keeps working with the option off)
            loss = self.loss(outputs, rgbs, mask, image_hw) if dssim_wanted(self.opt) else self.loss(outputs, rgbs, mask)
        if self.scaler is not None:
            self._arm_table_step()
            try:
                self.scaler.backward(loss)
            except BaseException:
                self.optimizer.disarm_in_backward()
                raise
        else:
            (loss * self.loss_scale).backward()
        if self.fused_adam:
            apply_optimizer_step(self)
        else:
            self.allreduce_grads()
            f = self.lr_factor()
            for g, base in zip(self.optimizer.param_groups, self.base_lrs):
                g['lr'] = base * f
            inv = 1.0 / (self.loss_scale * self.world_size)
            if inv != 1.0:
                torch._foreach_mul_([p.grad for p in self.model.parameters() if p.grad is not None], inv)
            self.optimizer.step()
            self.optimizer.zero_grad(set_to_none=False)
        self.global_step += 1
        return loss.detach(), outputs

    def train_step_graphed(self, rays_o, rays_d, rgbs, mask, **render_kw):
        """Buffer ownership: everything a captured graph reads is either one of the view's four resident tensors (pinned by the cache entry), a
        parameter / its .grad / optimiser state (never reallocated), an allocation made during capture (graph pool), or a cached scratch buffer
        (_lib.ScratchCache) — and the graph cache is flushed whenever one of those is reallocated: self._graph_gen is the _lib.scratch_generation()
        the cached graphs are valid for.

        train_step with render + loss + backward replayed as ONE hipGraph per view (opt-in).  A view is recognised by the addresses of its four
        resident tensors (a dataset keeps its rays on the GPU and hands the same tensors out every epoch); the first visit runs two eager steps
        (allocations, workspaces) and captures the third, later visits replay it.  The optimiser step stays eager: its learning rate is a host-side
        scalar that changes every step.  The GPU time is the eager step's (the step is GPU-bound: DESIGN.md section 6); what the graph buys is the
        host — 0.18 instead of 0.79 ms of enqueue per step (scratch/graph_probe.py) — i.e. immunity against a slow or shared host.
        Fused Adam with the on-device loss scaler, no --batch_rays subsampling; data-parallel trainers too (round 6): the gradient exchange and
        the optimiser step run eagerly after the replay — what matters under `--scaling strong`, where a rank's 2048-ray share of a view is 0.5 ms
        of kernels behind 1 ms of eager enqueue (profiles/r06_batch_sweep.json).  -> (loss, None): the loss is a static tensor that the
        next replay of the same view overwrites; the per-ray outputs stay inside the graph's memory pool."""
        if not (self.fused_adam and self.scaler is not None) or int(getattr(self.opt, 'batch_rays', -1) or -1) > 0:
            raise ValueError("train_step_graphed: fused Adam with the dynamic loss scaler, no batch_rays")
        from ._lib import scratch_generation
        image_hw = render_kw.pop('image_hw', None)
        dssim_check(self.opt, image_hw, rays_o.reshape(-1, 3).shape[0])
        image_hw = tuple(int(v) for v in image_hw) if image_hw is not None else None
        if ray_reg_wanted(self.opt):
            render_kw.setdefault('ray_reg', True)
        tensors = (rays_o, rays_d, rgbs, mask)
        key = tuple((t.data_ptr(), tuple(t.shape), t.dtype) for t in tensors) + (tuple(sorted(render_kw.items())), image_hw)
        cache = self.__dict__.setdefault('_graphs', {})
        if cache and self._graph_gen != scratch_generation():
            # a grow-on-demand workspace (scatter records, partial-gradient rows) was reallocated since a cached graph was captured — e.g. by an
            # eval_step on a larger view: it holds the freed buffer's address.  Drop them all (and their pool); every view recaptures.
            cache.clear()
            self.__dict__.pop('_graph_pool', None)
        ent = cache.get(key)
        if ent is None:
            gen0 = scratch_generation()
            for _ in range(2):
                self.train_step(rays_o, rays_d, rgbs, mask, image_hw=image_hw, **render_kw)
            torch.cuda.synchronize()
            self.model.train()
            graph = torch.cuda.CUDAGraph()
            self._watch_scaler()
            try:
                with torch.cuda.graph(graph, pool=self.__dict__.get('_graph_pool')), packed_weights_window(self.model, self.opt):
                    with torch.autocast('cuda', dtype=torch.float16, enabled=self.fp16):
                        outputs = self.model.render(rays_o, rays_d, staged=False, perturb=True, force_all_rays=True,
                                                    **dict(render_kw, fg_bg=render_kw.get('fg_bg', getattr(self, 'needs_fg_bg', False))))
                        loss = self.loss(outputs, rgbs, mask, image_hw) if dssim_wanted(self.opt) else self.loss(outputs, rgbs, mask)
                    self.scaler.backward(loss)
                    loss = loss.detach()
            finally:
                self.scaler.watch(False)
            if scratch_generation() != gen0 and cache:
                # The workspaces are keyed by (device, stream): the ones a graph references belong to the CAPTURE stream and are allocated
                # (graph pool) or re-grown during a capture.  This view grew one — in its warm-up or in its capture — so every graph captured
                # before holds the address of a block that went back to the shared pool and may alias this view's allocations: drop them
                # (they recapture on their next visit); the new graph, captured against the buffers as they are now, stays.
                cache.clear()
            self._graph_pool = graph.pool()
            self._graph_gen = scratch_generation()                   # (entries that survived are valid for the current generation too)
            ent = cache[key] = (graph, loss, tensors)                # (the tensors keep the captured addresses alive)
        self.model.train()
        self._inf_folded = inf_check_is_folded(self)                 # (the captured kernels carry the pointer they were captured with: this scaler's)
        ent[0].replay()
        apply_optimizer_step(self)
        self.global_step += 1
        return ent[1], None


def train_one_epoch(trainer, views, shard=None, log=None):
    """Loop body of Trainer_Nerf.train_one_epoch (nerf/utils_init_nerf.py:577-671) over an indexable of view tuples
    (rgbs, mask, rays_o, rays_d, H, W, img_path) — e.g. customnerf_amd.nerf.provider.NerfstudioScene — for ReconTrainer or EditTrainer:
    occupancy refresh every `opt.update_extra_interval` steps on the march path (:601-606), one optimiser step per view, mean loss.
    shard = (rank, world): view-parallel data parallelism, rank r takes views r, r + world, ... (the reference uses a DistributedSampler)."""
    model, opt = trainer.model, trainer.opt
    rank, world = shard if shard is not None else (0, 1)
    model.train()
    total, n = 0.0, 0
    for i in range(rank, len(views), world):
        if getattr(model, 'cuda_ray', False) and trainer.global_step % getattr(opt, 'update_extra_interval', 16) == 0:
            with torch.autocast('cuda', dtype=torch.float16, enabled=trainer.fp16):
                model.update_extra_state()
        data = views[i]
        if hasattr(trainer, 'train_step_editing'):                     # EditTrainer
            loss, loss_dict = trainer.train_step(data)
        else:
            rgbs, mask, rays_o, rays_d, H, W, _ = data
            extra = dict(image_hw=(int(H), int(W))) if dssim_wanted(opt) else {}    # the D-SSIM term reads the rays as the H x W view they are
            loss, _ = trainer.train_step(rays_o, rays_d, rgbs, mask, num_steps=opt.num_steps, upsample_steps=opt.upsample_steps,
                                         dt_gamma=getattr(opt, 'dt_gamma', 0), max_steps=opt.max_steps, **extra)
        total = total + loss                                           # stays on the device: no per-step host sync
        n += 1
    avg = float(total) / max(n, 1)
    if log is not None:
        log(f"==> Finished epoch: average_loss {avg:.6f} over {n} views, lr x{trainer.lr_factor():.4f}")
    return avg
