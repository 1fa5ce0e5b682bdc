"""NeRFRenderer — counterpart of the hot-path part of the reference's nerf/renderer.py.

Implemented (reference lines): sample_pdf (21-55), NeRFRenderer.__init__ (199-243), reset_extra_state (266-276),
run (278-405), weights_sum_i (407-474), run_cuda (597-718), update_extra_state (1658-1715), render (1719-1733),
convert_sigma_samples_to_ply (128-196) and the density_mesh hook (251) as NeRFRenderer.extract_mesh / save_mesh (marching cubes in mesh.hip).
render_depth (metric depth maps; no reference counterpart) feeds extract_mesh(tsdf=...), the TSDF fusion of mesh_tsdf.hip.
The mesh export methods are documented here and implemented in nerf/mesh_export.py.
Out of scope: the SDF/NeuS paths, the unused run_cuda2 / render_cuda duplicates.
Every function here ends in HIP kernels (render.hip, raymarching.hip, occupancy.hip): there is no torch restatement of the
reference's bodies in the product — that lives in oracle/torch_oracle.py, for the tests.

Reference defects handled deliberately (SURVEY.md "Known reference defects"):
  * run_cuda reads `opt.bg_color` which argparse never defines -> read with getattr(..., None);
  * run_cuda feeds 4-channel rgb+confidence rows to a stride-3 compositor -> our compositor takes the row stride;
  * run() with upsample_steps == 0 referenced an undefined name -> handled;
  * the output-dead density pass over the fine samples (renderer.py:353) is skipped unless
    `opt.eval_fine_density` asks for it (output-identical, tests/test_oracle_golden.py proves it on the reference).
"""
import inspect
import math

import numpy as np
import torch
import torch.nn as nn

from .. import raymarching, mesh as _mesh
from .._lib import lib, check, ptr, stream, require_cuda
from . import render_ops, mesh_export as _export


def sample_pdf(bins, weights, n_samples, det=False, u=None):
    """The reference's `sample_pdf(bins, weights, n_samples, det)` (renderer.py:21-55) on the HIP kernel k_sample_pdf: bins [B, T],
    weights [B, T-1] -> [B, n_samples].  `u` [B, n_samples] replays the random draw of :37 (drawn here with torch.rand when training).
    run() does not come through here — its resampling is fused with the merge (render_ops.sample_fine_merge)."""
    require_cuda(bins, weights, u)
    bins, weights = bins.contiguous().float(), weights.contiguous().float()
    B, T = bins.shape
    if weights.shape != (B, T - 1):
        raise ValueError(f"sample_pdf: weights must be [B, {T - 1}] for bins [B, {T}]")
    if not det and u is None:
        u = torch.rand(B, n_samples, device=bins.device)
    out = torch.empty(B, n_samples, dtype=torch.float32, device=bins.device)
    check(lib.cnerf_sample_pdf(ptr(bins), ptr(weights), None if det else ptr(u.contiguous().float()), B, T, int(n_samples), ptr(out), stream()), "sample_pdf")
    return out


def convert_sigma_samples_to_ply(input_3d_sigma_array, voxel_grid_origin, volume_size, ply_filename_out, level=5.0, offset=None, scale=None):
    """renderer.py:128-196 with the marching cubes on the GPU (mesh.marching_cubes) and the PLY written by mesh.write_ply.
    input_3d_sigma_array [X, Y, Z] (NumPy array or tensor); volume_size = the spacing per axis; the written points are
    (origin + verts) / scale - offset.  Returns skimage-style (verts, faces, normals) NumPy arrays, verts = index * spacing (no origin)."""
    vol = input_3d_sigma_array
    vol = (vol if torch.is_tensor(vol) else torch.from_numpy(np.ascontiguousarray(vol))).float()
    if not vol.is_cuda:
        vol = vol.cuda()
    verts, faces, normals = _mesh.marching_cubes(vol, level, spacing=tuple(volume_size), origin=(0.0, 0.0, 0.0))
    verts, faces, normals = verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy()
    mesh_points = verts + np.asarray(voxel_grid_origin, dtype=np.float32)
    if scale is not None:
        mesh_points = mesh_points / scale
    if offset is not None:
        mesh_points = mesh_points - offset
    _mesh.write_ply(ply_filename_out, mesh_points, faces)
    return verts, faces, normals


def normals_from_gradient(grad):
    """[..., 3] density gradient -> unit normals -grad / |grad|, zero where |grad|^2 < 1e-20 (safe_normalize's epsilon,
    provider_utils.py:125-126; there the division by sqrt(eps) leaves a vector of length < 1, here it is the zero vector, as in
    cnerf_composite_normals)"""
    q = (grad * grad).sum(-1, keepdim=True)
    return torch.where(q >= 1e-20, -grad / q.clamp_min(1e-20).sqrt(), torch.zeros_like(grad))


class _Lazy:
    """a result-dict entry that is computed on first access (entries the training loop never reads cost no launches)"""
    __slots__ = ('fn', 'value', 'done')

    def __init__(self, fn):
        self.fn, self.value, self.done = fn, None, False

    def get(self):
        if not self.done:
            self.value, self.done, self.fn = self.fn(), True, None
        return self.value


class _LazyResults(dict):
    """dict whose _Lazy values are materialised by [] / get / items / values (keys, `in` and len behave as for a plain dict)"""

    def __getitem__(self, k):
        v = dict.__getitem__(self, k)
        if isinstance(v, _Lazy):
            v = v.get()
            dict.__setitem__(self, k, v)
        return v

    def get(self, k, default=None):
        return self[k] if k in self else default

    def items(self):
        return [(k, self[k]) for k in dict.keys(self)]

    def values(self):
        return [self[k] for k in dict.keys(self)]


class NeRFRenderer(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.bound = opt.bound
        self.cascade = 1 + math.ceil(math.log2(opt.bound))
        self.grid_size = 128
        self.cuda_ray = opt.cuda_ray
        self.min_near = opt.min_near
        self.density_thresh = opt.density_thresh

        aabb_train = torch.FloatTensor([-opt.bound, -opt.bound, -opt.bound, opt.bound, opt.bound, opt.bound])
        self.register_buffer('aabb_train', aabb_train)
        self.register_buffer('aabb_infer', aabb_train.clone())
        self.register_buffer('aabb_train_bg', 2 * aabb_train.clone())
        self.register_buffer('aabb_infer_bg', 2 * aabb_train.clone())

        if self.cuda_ray:                                                        # renderer.py:230-243
            self.register_buffer('density_grid', torch.zeros([self.cascade, self.grid_size ** 3]))
            self.register_buffer('density_bitfield', torch.zeros(self.cascade * self.grid_size ** 3 // 8, dtype=torch.uint8))
            self.mean_density = 0
            self.iter_density = 0
            self.register_buffer('step_counter', torch.zeros(16, 2, dtype=torch.int32))
            self.mean_count = 0
            self.local_step = 0

    def forward(self, x, d):
        raise NotImplementedError()

    def density(self, x):
        raise NotImplementedError()

    def reset_extra_state(self):
        if not self.cuda_ray:
            return
        self.density_grid.zero_()
        self.mean_density = 0
        self.iter_density = 0
        self.step_counter.zero_()
        self.mean_count = 0
        self.local_step = 0

    # ------------------------------------------------------------------------------------------ run (the path `-O2` takes)
    def run(self, rays_o, rays_d, num_steps=128, upsample_steps=128, light_d=None, ambient_ratio=1.0, shading='albedo',
            bg_color=None, perturb=False, _draws=None, normals=False, ray_reg=False, **kwargs):
        """renderer.py:278-405.  rays_o, rays_d [B,N,3] (B == 1) -> result dict, on the fused HIP kernels (no torch fallback: CPU
        tensors raise).  `_draws` = dict(light, z, u) replays the RNG draws of :305, :317 and sample_pdf:37 (tests).
        The reference fills its result dict only under `opt.train_conf` (:383-405): without it the dict is empty here too.
        normals=True adds the field's normals (density_gradient of the subclass; csrc/field_normal.hip), detached even when grad is enabled:
        'normal_map' [*prefix, 3] = sum w n (renderer.py:469-470; 'fg' and 'bg' get theirs from their own weights), 'orient' [*prefix] =
        sum w max(0, n . d)^2 (the summand of loss_orient, :428, per ray) and 'normal' [N, S, 3], the per-sample normals in sorted order
        (computed on first access).  With the default no launch is added and no key.
        ray_reg=True adds the two regularisers of the sample weights (render_ops.ray_regularizers; one launch, one more in the backward):
        'distortion' and 'ray_entropy' [*prefix], differentiable, and the same two keys in 'fg' / 'bg' where those composites are computed.
        The entropy is gated by `opt.ray_reg_min_opacity` (default 0.1).  With the default no launch is added and no key."""
        require_cuda(rays_o, rays_d)
        if not getattr(self.opt, 'train_conf', 0):
            return {}
        if not (3 <= num_steps <= 128 and 2 <= upsample_steps <= 128):
            # (upsample_steps == 0 fails in the reference as well: `weights` is bound only inside `if upsample_steps > 0`, renderer.py:333-384)
            raise ValueError(f"run(): the sampling kernels take 3..128 coarse and 2..128 importance samples per ray (got {num_steps} + {upsample_steps}; "
                             "the reference's recipe is 64 + 64)")
        return self._run_fused(rays_o, rays_d, num_steps, upsample_steps, perturb, _draws, fg_bg=bool(kwargs.get('fg_bg', True)), normals=bool(normals),
                               ray_reg=bool(ray_reg))

    def _dirs_twice(self, rays_d):
        """[d | d] for the split sample list, cached per view: a dataset's ray directions are resident tensors that come back every epoch
        (provider.py keeps them on the GPU), so the concatenation launch is paid once per view, not once per step"""
        if torch.cuda.is_current_stream_capturing():
            # hipGraph capture (trainer.train_step_graphed): the concatenation becomes a node of the graph and its result lives in the graph's
            # own memory pool — a cached tensor's address would be baked into the graph and outlive its eviction from the 64-entry cache
            return torch.cat([rays_d, rays_d], 0)
        cache = self.__dict__.setdefault('_dirs2_cache', {})
        key = (rays_d.data_ptr(), rays_d._version, tuple(rays_d.shape))
        ent = cache.get(key)
        if ent is None:
            if len(cache) >= 64:
                cache.pop(next(iter(cache)))
            ent = (rays_d, torch.cat([rays_d, rays_d], 0))               # the source reference pins the key's storage
            cache[key] = ent
        return ent[1]

    def _field_all(self, xyz, rays_d, S):
        """sigma [P], rgb+confidence [P, 4] of P = N*S samples (S consecutive samples share a ray direction) from a subclass forward()"""
        if getattr(self, 'supports_dir_group', False):
            sigmas, rgbc, _ = self(xyz, rays_d, dir_group=S)
        else:
            sigmas, rgbc, _ = self(xyz, rays_d.repeat_interleave(S, dim=0))
        if rgbc.shape[-1] != 4:
            raise ValueError("run() with opt.train_conf needs forward() to return rgb + 1 confidence channel (network_grid.py:126-129)")
        return sigmas.reshape(-1), rgbc.reshape(-1, 4)

    def _run_fused(self, rays_o, rays_d, num_steps, upsample_steps, perturb, _draws=None, fg_bg=True, normals=False, ray_reg=False):
        """run() on the fused kernels: 2 sampling launches + 2 field launches (+1 gather each) + 1 composite launch.
        Same result dict as run(); RNG draws keep the reference's order (rand(N,T) then rand(N,t)).
        fg_bg=False (the reconstruction trainer, whose loss reads the first composite only): the edit-region / background composites are not
        computed and the result dict has no 'fg' / 'bg' entries."""
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3).float()
        rays_d = rays_d.contiguous().view(-1, 3).float()
        N = rays_o.shape[0]
        device = rays_o.device
        draws = _draws or {}
        aabb = self.aabb_train if self.training else self.aabb_infer
        S = num_steps + upsample_steps
        soft, thr = bool(getattr(self.opt, 'soft_mask', False)), float(getattr(self.opt, 'conf_thr', 0.5))
        dbg, dmask = bool(getattr(self.opt, 'detach_bg', False)), bool(getattr(self.opt, 'detach_mask_from_field', False))
        split = (num_steps == upsample_steps and getattr(self.opt, 'split_eval', True) and getattr(self, 'supports_split_eval', False)
                 and not getattr(self.opt, 'eval_fine_density', False))
        grad_on = torch.is_grad_enabled()
        if not split:
            nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, self.min_near)
        with torch.no_grad():
            noise = None
            both = None
            blockwise = False
            if perturb and self.training and 'z' not in draws and 'u' not in draws:
                # rand(N,T) then rand(N,t) (renderer.py:317, :37) drawn by one generator launch: the first N*T values are the jitter
                both = torch.rand(N * (num_steps + upsample_steps), device=device)
            if perturb:
                noise = (draws['z'].to(device).contiguous() if 'z' in draws else
                         (both[:N * num_steps].view(N, num_steps) if both is not None else torch.rand(N, num_steps, device=device)))
            if self.training:
                u_draw = lambda: (draws['u'].to(device).contiguous() if 'u' in draws else
                                  (both[N * num_steps:].view(N, upsample_steps) if both is not None else torch.rand(N, upsample_steps, device=device)))
            else:
                u_draw = lambda: None                                         # det=True (sample_pdf :33-35)
            if split:
                # sample list = [coarse block N*T | fine block N*t]; the coarse block's grid features are gathered once (density pass) and
                # stay in `enc` for the full evaluation; the sorted order only exists as an index (src) for the compositing kernels.
                Pc, P = N * num_steps, N * S
                xyz_list = torch.empty(P, 3, dtype=torch.float32, device=device)
                enc, unit = self.split_buffers(P, device)
                bnd = float(self.opt.bound)                                  # the samplers also write the grid's [0,1] coordinates (no elementwise pass)
                # near_far_from_aabb (:297) rides on the coarse sampler's launch
                nears, fars, z_vals, xyz_c = render_ops.sample_coarse_aabb(rays_o, rays_d, aabb.contiguous().float(), self.min_near, num_steps, noise,
                                                                           xyz_list[:Pc].view(N, num_steps, 3), unit[:Pc].view(N, num_steps, 3), bnd)
                self.split_encode(enc, unit, xyz_list[:Pc], 0, unit_ready=True)
                blockwise = bool(getattr(self.opt, 'blockwise_field', True)) and self._fused_cfg()[2] == 4
                if blockwise:
                    # full evaluation of the coarse block right away: its sigma drives the importance sampling and its colours are the
                    # coarse half of the final evaluation — no density-only pass, no second visit of these rows
                    sig_all, rgbc_all = self.split_outputs(P, device)
                    self.split_forward_rows(enc, 0, xyz_list[:Pc], rays_d, num_steps, sig_all, rgbc_all)
                    sig_c = sig_all[:Pc]
                else:
                    sig_c = self.split_density(enc, xyz_list[:Pc])
                z_all, xyz_f, src = render_ops.sample_fine_merge_split(rays_o, rays_d, nears, fars, aabb, z_vals, sig_c, upsample_steps, u_draw(),
                                                                        xyz_fine_out=xyz_list[Pc:].view(N, upsample_steps, 3),
                                                                        unit_fine_out=unit[Pc:].view(N, upsample_steps, 3), bound=bnd)
                self.split_encode(enc, unit, xyz_list[Pc:], Pc, unit_ready=True, importance=True)
                if blockwise:
                    self.split_forward_rows(enc, Pc, xyz_list[Pc:], rays_d, upsample_steps, sig_all, rgbc_all)
            else:
                z_vals, xyzs = render_ops.sample_coarse(rays_o, rays_d, nears, fars, aabb, num_steps, noise)
                sig_c = self.density(xyzs.view(-1, 3))['sigma'].float().contiguous()
                z_all, xyz_all = render_ops.sample_fine_merge(rays_o, rays_d, nears, fars, aabb, z_vals, sig_c, upsample_steps, u_draw())
                if getattr(self.opt, 'eval_fine_density', False):
                    self.density(xyz_all.view(-1, 3))
        if split:
            # both blocks hold num_steps samples per ray, so "one direction per num_steps consecutive samples" covers the list with [d | d]
            dirs2 = self._dirs_twice(rays_d)
            if blockwise:
                sig_l, rgbc_l = self.split_attach(enc, unit, xyz_list, dirs2, num_steps, sig_all, rgbc_all)
            else:
                sig_l, rgbc_l = self.split_forward(enc, unit, xyz_list, dirs2, num_steps)
            # early termination of the backward (north_star; the reference's own is `T < T_thresh` on its march path): only where the gradients
            # go into the half-precision fused field, whose backward rounds them to half anyway
            flush = bool(grad_on and getattr(self.opt, 'early_termination', True) and self._fused_cfg() and self._half())
            out_ray = render_ops.composite_run_indexed(sig_l, rgbc_l, z_all, src, nears, fars, num_steps, soft, thr, dbg, dmask, flush_half_zero=flush,
                                                       variants=7 if fg_bg else 1)
            # per-sample by-products (weights, sorted-order sigma / rgbc copies, detached): a second launch, only if somebody reads them
            aux = _Lazy(lambda: render_ops.composite_run_indexed_aux(sig_l, rgbc_l, z_all, src, nears, fars, num_steps, soft, thr))
            weights_of = lambda v: _Lazy(lambda: aux.get()[0][v])
            sigma_e = _Lazy(lambda: aux.get()[1].view(N, S, 1))
            rgbs_e = _Lazy(lambda: aux.get()[2].view(N, S, 4)[..., :3])
            conf_of = lambda: aux.get()[2].view(N, S, 4)[..., 3:4]
        else:
            sigmas, rgbc = self._field_all(xyz_all.view(-1, 3), rays_d, S)
            out_ray, out_w = render_ops.composite_run(sigmas.view(N, S), rgbc.view(N, S, 4), z_all, nears, fars, num_steps, soft, thr, dbg, dmask)
            weights_of = lambda v: out_w[v]
            sigma_e, rgbs_e = sigmas.view(N, S, 1), rgbc.view(N, S, 4)[..., :3]
            conf_of = lambda: rgbc.view(N, S, 4)[..., 3:4]
        mask = _Lazy(lambda: (nears < fars).reshape(*prefix))

        def pack(v):
            r = out_ray[v]
            return _LazyResults({'image': r[:, 0:3].reshape(*prefix, 3), 'depth': r[:, 3].reshape(*prefix), 'weights_sum': r[:, 4],
                                 'render_mask': r[:, 5].reshape(*prefix, 1), 'weights': weights_of(v), 'mask': mask})
        results = pack(0)
        results['sigma'] = sigma_e
        results['rgbs'] = rgbs_e
        if getattr(self.opt, 'soft_mask', False):
            thr_ = self.opt.conf_thr
            results['edit_mask'] = _Lazy(lambda: torch.sigmoid((conf_of().detach() - thr_) * 100))
        else:
            results['edit_mask'] = _Lazy(lambda: conf_of().detach() > 0.5)
        results['z_vals'] = z_all
        results['_out_ray'] = out_ray                                        # [3, N, 6] raw composite output (trainer.ReconTrainer's fused loss)
        if fg_bg or not split:                                               # (fg_bg=False: the two composites were not computed — no such keys)
            results['fg'] = pack(1)
            results['bg'] = pack(2)
        if ray_reg:
            # distortion / ray entropy of the weights of every composite that was computed: the same samples, through the same index
            if split:
                reg_in = (sig_l, rgbc_l, z_all, src)
            else:
                reg_in = (sigmas, rgbc, z_all, None)
            reg = render_ops.ray_regularizers(*reg_in, nears, fars, num_steps, soft, thr, dbg, variants=7 if 'fg' in results else 1,
                                              min_opacity=float(getattr(self.opt, 'ray_reg_min_opacity', 0.1)))
            for v, r in enumerate((results, results.get('fg'), results.get('bg'))[:3 if 'fg' in results else 1]):
                r['distortion'] = reg[v, :, 0].reshape(*prefix)
                r['ray_entropy'] = reg[v, :, 1].reshape(*prefix)
        if normals:
            # the gradient of the whole sample list: on the split path from the resident features and grid coordinates (no second gather)
            with torch.no_grad():
                if split:
                    grad_x = self.split_density_gradient(enc, unit, xyz_list)[1]
                    order = src
                else:
                    grad_x = self.density_gradient(xyz_all.view(-1, 3))['grad']
                    order = None
                V = 3 if 'fg' in results else 1
                w = [weights_of(v) for v in range(V)]
                w = torch.stack([x.get() if isinstance(x, _Lazy) else x for x in w])
                nmap, orient = render_ops.composite_normals(w, order, grad_x, rays_d)
            for v, r in enumerate((results, results.get('fg'), results.get('bg'))[:V]):
                r['normal_map'] = nmap[v].reshape(*prefix, 3)
                r['orient'] = orient[v].reshape(*prefix)
            results['normal'] = _Lazy(lambda: normals_from_gradient(grad_x if order is None else grad_x[order.reshape(-1).long()]).view(N, S, 3))
        return results

    def weights_sum_i(self, sample_dist, sigmas, normals, dirs, weights, z_vals, nears, fars, rgbs, prefix, masks=None,
                      bg_color=None, if_fg=False, is_all=False, num_steps=None):
        """One alpha composite with the reference's signature (renderer.py:407-474) on the compositing kernel of run() (its "all" variant
        takes sigma as given): sigmas [N,S(,1)], rgbs [N,S,3], masks [N,S,1] | None, z_vals [N,S], nears / fars / sample_dist [N,1].
        Differentiable in sigmas / rgbs / masks.  `num_steps` = (far - near) / sample_dist, the kernel's form of the last interval; when it is
        not passed it is recovered from the first ray that hits the box (one host read; rays with near >= far carry no interval)."""
        N, S = z_vals.shape
        nears, fars = nears.reshape(N).contiguous().float(), fars.reshape(N).contiguous().float()
        if num_steps is None:
            sd_ = sample_dist.reshape(-1).float().expand(N) if sample_dist.numel() in (1, N) else sample_dist.reshape(-1).float()[:N]
            ratio = torch.where((fars > nears) & (sd_ > 0), (fars - nears) / sd_.clamp_min(1e-30), torch.full_like(nears, -1.0))
            num_steps = int(torch.round(ratio.max()).item())         # every valid ray has the same (far - near) / sample_dist = the sample count
            if num_steps <= 0:
                raise ValueError("weights_sum_i: no ray intersects the box (near >= far everywhere); pass num_steps")
        conf = masks.reshape(N, S, 1).float() if masks is not None else torch.zeros(N, S, 1, device=z_vals.device)
        rgbc = torch.cat([rgbs.reshape(N, S, 3).float(), conf], dim=-1)
        detach_bg = bool(is_all and getattr(self.opt, 'detach_bg', False))                           # :409-418
        out_ray, out_w = render_ops.composite_run(sigmas.reshape(N, S).float(), rgbc, z_vals.contiguous().float(), nears, fars, num_steps,
                                                  True, float(getattr(self.opt, 'conf_thr', 0.5)), detach_bg,
                                                  bool(getattr(self.opt, 'detach_mask_from_field', False)))
        r = out_ray[0]
        results = {}
        image = r[:, 0:3].reshape(*prefix, 3)
        if if_fg and bg_color is not None:                                                            # :451-453
            results['black_image'] = image
            image = image + (1 - r[:, 4]).unsqueeze(-1).reshape(*prefix, 1) * bg_color
        results['image'] = image
        if getattr(self.opt, 'train_conf', 0) and masks is not None:
            results['render_mask'] = r[:, 5].reshape(*prefix, 1)
        results['depth'] = r[:, 3].reshape(*prefix)
        results['weights_sum'] = r[:, 4]
        results['weights'] = out_w[0]
        results['mask'] = (nears < fars).reshape(*prefix)
        return results

    # ------------------------------------------------------------------------------------------ run_cuda (occupancy march)
    def run_cuda(self, rays_o, rays_d, dt_gamma=0, light_d=None, ambient_ratio=1.0, shading='albedo', bg_color=None,
                 perturb=False, force_all_rays=False, max_steps=1024, T_thresh=1e-4, _noises=None, normals=False, **kwargs):
        """renderer.py:597-718: occupancy-grid march.  Training: one compacted sample list per batch (march_rays_train ->
        field -> composite_rays_train); inference: the alive-ray loop of :661-688 with device-side compaction.
        normals=True raises NotImplementedError: normal maps exist on run() only."""
        if kwargs.get('ray_reg', False):
            raise ValueError("run_cuda(ray_reg=True): the distortion / ray-entropy regularisers exist on run() only (a model with opt.cuda_ray "
                             "off); the occupancy march keeps no per-ray sample weights to regularise")
        if normals:
            raise NotImplementedError("run_cuda(normals=True): normal maps are composited by run() only; the occupancy march has none "
                                      "(use a model with opt.cuda_ray off, or model.normal(x) per point)")
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.cuda().contiguous().view(-1, 3)
        rays_d = rays_d.cuda().contiguous().view(-1, 3)
        aabb = self.aabb_train if self.training else self.aabb_infer
        # the reference passes no min_near here: the wrapper's default 0.2 applies (:612-613)
        nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb)
        results = {}
        if self.training:
            weights_sum, depth, image = self._march_train(rays_o, rays_d, nears, fars, dt_gamma, perturb, force_all_rays, max_steps, T_thresh, _noises, results)
        else:
            weights_sum, depth, image = self._march_infer(rays_o, rays_d, nears, fars, dt_gamma, perturb, max_steps, T_thresh, light_d, ambient_ratio, shading)
        bg = getattr(self.opt, 'bg_color', None)                    # read by the reference (:694) but never defined by its argparse
        if bg:
            bg = torch.as_tensor(np.asarray(bg, dtype=np.float32), device=image.device).reshape(1, -1)
            image = image + (1 - weights_sum).unsqueeze(-1) * bg
        results.update(image=image.view(*prefix, 3), depth=depth.view(*prefix), weights_sum=weights_sum.reshape(*prefix),
                       mask=(nears < fars).reshape(*prefix))
        return results

    def _march_train(self, rays_o, rays_d, nears, fars, dt_gamma, perturb, force_all_rays, max_steps, T_thresh, noises, results):
        """:617-635.  The per-call sample counter is one slot of the 16-entry ring `step_counter` (mean_count is their average, update_extra_state)."""
        counter = self.step_counter[self.local_step % 16]
        counter.zero_()
        self.local_step += 1
        xyzs, dirs, deltas, rays = raymarching.march_rays_train(rays_o, rays_d, self.bound, self.density_bitfield, self.cascade, self.grid_size,
                                                                nears, fars, counter, self.mean_count, perturb, 128, force_all_rays, dt_gamma,
                                                                max_steps, noises=noises)
        sigmas, rgbs, _ = self(xyzs, dirs)
        results['rays'] = rays
        results['num_points'] = xyzs.shape[0]
        return raymarching.composite_rays_train(sigmas, rgbs.float(), deltas, rays, T_thresh)

    def _march_infer(self, rays_o, rays_d, nears, fars, dt_gamma, perturb, max_steps, T_thresh, light_d, ambient_ratio, shading):
        """:637-688.  Every round advances each alive ray by n_step occupied samples, accumulates in place and compacts the alive list on the
        device (`rays_alive[rays_alive >= 0]` of :684 as a ballot + scan kernel); the only host read per round is the alive count that sizes
        the next round's launches."""
        N, device = rays_o.shape[0], rays_o.device
        acc = torch.zeros(5 * N, dtype=torch.float32, device=device)                # weights_sum | depth | rgb: one zero-fill, three views
        weights_sum, depth, image = acc[:N], acc[N:2 * N], acc[2 * N:].view(N, 3)
        alive = torch.arange(N, dtype=torch.int32, device=device)
        alive_next = torch.empty_like(alive)
        count = torch.zeros(1, dtype=torch.int32, device=device)
        rays_t = nears.clone()
        n_alive, done = N, 0
        while done < max_steps and n_alive > 0:
            n_step = max(min(N // n_alive, 8), 1)                                   # :671
            xyzs, dirs, deltas = raymarching.march_rays(n_alive, n_step, alive, rays_t, rays_o, rays_d, self.bound, self.density_bitfield,
                                                        self.cascade, self.grid_size, nears, fars, 128, perturb and done == 0, dt_gamma, max_steps)
            sigmas, rgbs, _ = self(xyzs, dirs, light_d, ratio=ambient_ratio, shading=shading)
            raymarching.composite_rays(n_alive, n_step, alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, T_thresh)
            raymarching.compact_rays_alive(alive, n_alive, alive_next, count)
            alive, alive_next = alive_next, alive
            n_alive = int(count.item())
            done += n_step
        return weights_sum, depth, image

    # ------------------------------------------------------------------------------------------ occupancy grid refresh
    @property
    def mean_density(self):
        """mean of the valid cells after the last refresh (renderer.py:1710); kept on the device by update_extra_state, read on demand"""
        md = self.__dict__.get('_mean_density', 0)
        return float(md[0]) if torch.is_tensor(md) else md

    @mean_density.setter
    def mean_density(self, v):
        self.__dict__['_mean_density'] = v

    @torch.no_grad()
    def update_extra_state(self, decay=0.95, S=128, _rand=None):
        """renderer.py:1658-1715 as kernels (csrc/occupancy.hip): per cascade, jittered cell-centre queries -> density -> EMA-max into
        `density_grid` (Morton order); then mean density, threshold min(mean, density_thresh) and packbits in one go, all on the device.
        `S` (the reference's chunk size) is accepted and ignored: a cascade's 128^3 queries are one batch.  `_rand` = list of [H^3, 3] U[0,1)
        tensors, one per cascade, replaying the `torch.rand_like` draws of :1695 (tests).  The only host read is the 16-slot sample-count
        ring that sizes the next march_rays_train calls (:1714-1716)."""
        if not self.cuda_ray:
            return
        H, dev = self.grid_size, self.density_bitfield.device
        n = H ** 3
        nblk = (n + 255) // 256
        partials = torch.empty(self.cascade * nblk, 2, dtype=torch.float64, device=dev)
        xyzs = torch.empty(n, 3, dtype=torch.float32, device=dev)
        for cas in range(self.cascade):
            bound = min(2 ** cas, self.bound)
            half = bound / H
            rnd = (_rand[cas].to(dev) if _rand is not None else torch.rand(n, 3, device=dev)).contiguous().float()
            check(lib.cnerf_occupancy_points(ptr(rnd), H, float(bound), float(half), ptr(xyzs), stream()), "occupancy_points")
            sigmas = self.density(xyzs)['sigma'].reshape(-1).float().contiguous()
            check(lib.cnerf_occupancy_update(ptr(sigmas), H, float(decay), ptr(self.density_grid[cas]), ptr(partials[cas * nblk:]), stream()), "occupancy_update")
        state = torch.empty(2, dtype=torch.float32, device=dev)
        check(lib.cnerf_occupancy_finalize_pack(ptr(partials), self.cascade * nblk, float(self.density_thresh), ptr(self.density_grid),
                                                self.density_bitfield.numel(), ptr(state), ptr(self.density_bitfield), stream()), "occupancy_finalize_pack")
        self.mean_density = state
        self.iter_density += 1
        total_step = min(16, self.local_step)
        if total_step > 0:
            self.mean_count = self._mean_sample_count(total_step)
        self.local_step = 0

    def _mean_sample_count(self, total_step):
        """average samples per march_rays_train call over the last `total_step` calls (:1714-1716); data-parallel ranks average it too, so
        that every rank sizes its sample budget alike.  That makes update_extra_state a COLLECTIVE under torch.distributed (every rank must
        call it); `opt.sync_mean_count = False` keeps it rank-local (e.g. a rank-0-only evaluation that refreshes the occupancy grid)."""
        tot = self.step_counter[:total_step, 0].sum().float()
        import torch.distributed as dist
        if getattr(self.opt, 'sync_mean_count', True) and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            from .. import _coll
            _coll.all_reduce(tot)
            tot = tot / dist.get_world_size()
        return int(tot.item() / total_step)

    # ------------------------------------------------------------------------------------------ mesh export (the reference's density_mesh hook, :251)
    # The field's side of it lives here (_mesh_lattice, _mesh_sigma, density_volume); the pipeline is nerf/mesh_export.py, and the methods
    # below that carry its API and documentation delegate to it.
    def _mesh_lattice(self, resolution, aabb):
        aabb = (self.aabb_infer if aabb is None else torch.as_tensor(aabb, dtype=torch.float32)).detach().float().cpu().reshape(6)
        lo, hi = aabb[:3], aabb[3:]
        if resolution < 2 or not bool((hi > lo).all()):
            raise ValueError(f"extract_mesh: need resolution >= 2 and a non-empty box, got {resolution} and {aabb.tolist()}")
        return lo, (hi - lo) / (resolution - 1)

    def _mesh_sigma(self, x, part='all', view_dir=(0.0, 0.0, -1.0)):
        """The field that mesh extraction takes the isosurface of, at positions x [m, 3] -> [m] float32 (density_volume's docstring says
        what `part` selects); elementwise, so the dense lattice and the bricks of a sparse extraction ask it alike."""
        if part not in ('all', 'fg', 'bg'):
            raise ValueError(f"extract_mesh: part must be 'all', 'fg' or 'bg', got {part!r}")
        if part == 'all':
            return self.density(x)['sigma'].reshape(-1).float()
        d = torch.tensor(view_dir, dtype=torch.float32, device=x.device).reshape(1, 3)
        sigma, rgbc = self(x, d.expand(len(x), 3).contiguous())[:2]
        if rgbc.shape[-1] < 4:
            raise ValueError("extract_mesh: part='fg' / 'bg' needs a field with a confidence channel (opt.train_conf)")
        sigma, conf = sigma.reshape(-1).float(), rgbc[:, 3].float()
        if bool(getattr(self.opt, 'soft_mask', False)):
            m = torch.sigmoid((conf - float(getattr(self.opt, 'conf_thr', 0.5))) * 100)
            return sigma * m if part == 'fg' else sigma * (1 - m)
        m = conf > 0.5
        return torch.where(m if part == 'fg' else ~m, sigma, torch.zeros_like(sigma))

    @torch.no_grad()
    def density_volume(self, resolution=256, aabb=None, chunk=2 ** 21, part='all', view_dir=(0.0, 0.0, -1.0)):
        """sigma on a resolution^3 lattice over `aabb` (default aabb_infer), [R, R, R] float32 in meshgrid('ij') order (z fastest).
        part 'all': self.density(x) (the fused density pass).  part 'fg' / 'bg': sigma and confidence from forward(x, view_dir), masked as
        run() masks the edit-region / background composites (renderer.py:386-395): soft mask sigmoid((conf - conf_thr) * 100) under
        opt.soft_mask, otherwise conf > 0.5; a field without a confidence channel raises ValueError."""
        R = int(resolution)
        lo, step = self._mesh_lattice(R, aabb)
        dev = self.aabb_infer.device
        lo, step = lo.to(dev), step.to(dev)
        n = R ** 3
        vol = torch.empty(n, dtype=torch.float32, device=dev)
        for s in range(0, n, chunk):
            i = torch.arange(s, min(s + chunk, n), device=dev, dtype=torch.int64)
            ijk = torch.stack([i // (R * R), (i // R) % R, i % R], dim=1).float()
            vol[s:s + len(i)] = self._mesh_sigma((lo + ijk * step).contiguous(), part, view_dir)      # which checks `part`
        return vol.view(R, R, R)

    _tsdf_options = staticmethod(_export.tsdf_options)                           # the names the host tests know them by
    _color_view_options = staticmethod(_export.color_view_options)

    @torch.no_grad()
    def extract_mesh(self, resolution=256, threshold=None, aabb=None, chunk=2 ** 21, part='all', view_dir=(0.0, 0.0, -1.0), color=False,
                     min_component_faces=0, keep_largest=False, simplify=0, target_faces=0, texture=0, smooth=0, smooth_lambda=0.5,
                     smooth_mu=-0.53, deviation=False, deviation_spacing=None, deviation_max_samples=1 << 26, ao=0,
                     texture_layout='uniform', bake_from='mesh', bake_reach=None, normal_map=False, sparse=False, sparse_probe=4,
                     tsdf=None, fill_holes=False, topology=False, color_views=None, remesh=None):
        """Isosurface sigma == threshold (default opt.density_thresh) of the field on a resolution^3 lattice over `aabb` (default
        aabb_infer): density_volume, then marching cubes on the device (mesh.marching_cubes).  color=True: forward(verts, -normals) gives
        each vertex the colour seen looking at the surface, as uint8 RGB.  -> dict of device tensors: verts [V, 3] float32 (world
        coordinates), faces [F, 3] int32 (wound outwards), normals [V, 3] (outward), colors [V, 3] uint8 or None, and the volume.
        Cleanup on the device (mesh.py, csrc/mesh_clean.hip), in this order, before the colours are sampled at the final vertices:
        min_component_faces > 0 drops the connected components with fewer faces (floaters); keep_largest=True keeps only the component with
        the most faces; smooth=k > 0 runs k Taubin iterations (smooth_lambda, smooth_mu; mesh.smooth, csrc/mesh_smooth.hip: boundary vertices
        stay, smooth_mu=0 is plain Laplacian smoothing), after which the normals are the area-weighted normals of the smoothed surface;
        simplify=k >= 2 clusters the vertices in cells of k lattice steps from the lattice's lower corner (mesh.simplify); target_faces > 0
        decimates by quadric edge collapse to that many faces (mesh.decimate; not with simplify, whose output need not be manifold).
        simplify and decimate carry the normals along, and color / texture look along them.  The defaults return the marching-cubes mesh
        as it is.
        texture=R > 0 bakes the field's colour, looking at the surface, into an R x R texture atlas of the final mesh (mesh.bake_texture,
        csrc/mesh_texture.hip): 'uvs' [F, 3, 2] float32 and 'texture' [R, R, 3] uint8 join the dict (both None with texture=0).
        texture_layout='uniform' gives every face the same texels; 'area' (R a power of two) sizes a face's cell by its longest edge, which
        is what a decimated mesh (target_faces), with its large faces on flat regions, wants; 'projected' groups the faces into charts by
        the axis of their normal and packs the projected charts (mesh.chart_plan, csrc/mesh_charts.hip): a texture that reads as an image
        and has seams only between charts.  'texture_layout' joins the dict.
        deviation=True reports what the lossy passes cost in geometry: 'deviation' joins the dict — mesh.distance(final mesh, the mesh as it
        stood after marching cubes and component removal), both directions (max, mean, rms per direction and 'hausdorff', in world units),
        sampled deviation_spacing apart (default: half the smallest lattice step; at most deviation_max_samples samples per direction,
        ValueError beyond), plus 'step', the lattice step, so that the error reads in voxels; None when neither smooth, simplify,
        target_faces nor remesh ran.  Without deviation=True the key is absent.
        ao=K > 0 adds 'ao' [V] float32 in [0, 1]: the per-vertex ambient occlusion of the final mesh from K rays per vertex
        (mesh.ambient_occlusion: the share of the rays that escape), a shading cue for geometry-only previews — render_mesh(colors=) shows
        it as grey.  It is never multiplied into colors or texture: the field's radiance already contains the scene's shading.  With ao=0
        the key is absent.
        bake_from='source' samples colour where the field was trained instead of on the decimated or smoothed faces, which lie off the
        isosurface by what 'deviation' reports: every texel of texture=R and every vertex of color=True is projected along the final mesh's
        normal onto the mesh as it stood after marching cubes and component removal (mesh.project_to_surface), at most bake_reach away
        (default: four times the largest lattice step; compare it with deviation['hausdorff'] — a reach below the deviation leaves texels
        unprojected, kind 0 below), and the field is asked there, looking against that surface's normal.  It is accepted when no lossy pass
        ran; the projections are then near zero.  'bake_kinds' joins the dict: [4] int64, the texels (with texture=0: the vertices) by the
        kind of their projection (0 nothing within reach, 1 along the normal, 2 against it, 3 the closest point past a rim).
        normal_map=True (needs texture=R) adds 'normal_map' [R, R, 3] uint8, an object-space normal map in the texture's layout: the
        normals of the full-resolution surface under bake_from='source' — the detail decimation removed, in a form a viewer can use —
        else the final mesh's own interpolated normals.  normal_map='tangent' makes it a tangent-space map, the kind glTF takes and the
        one that stays valid when the object is rotated or instanced (mesh.bake_texture(normal_map='tangent'), csrc/mesh_tangent.hip):
        'tangents' [F, 3, 4] float32, the frame of every face corner, joins the dict; without bake_from='source' the map is flat,
        (128, 128, 255).  'normal_space' ('object' or 'tangent') joins the dict with either.  With the defaults none of these keys is
        present.
        sparse=True extracts the same surface without the dense volume, which is what makes resolutions of 1024 and beyond affordable
        (the dense path holds resolution^3 values plus 6 bytes of workspace per point and refuses more than 2^31 points): the field is
        evaluated on a probe lattice of every sparse_probe-th point, then only in the bricks of 8^3 points around the surface found
        there, grown until the surface is covered (mesh.sparse_volume), and marching cubes runs over that brick list
        (mesh.marching_cubes_sparse, csrc/mesh_sparse.hip).  Same lattice, threshold and part, the same arithmetic: the mesh has the
        dense path's vertices and triangles, bit for bit, in brick order in place of lattice order — except that, with sparse_probe=k > 1,
        a surface component small enough to lie wholly between the probe points (as an extraction at resolution / k would lose it) can be
        missed; sparse_probe=1 misses nothing.  'volume' is then None and 'sparse' joins the dict: {'bricks', 'evaluations', 'rounds',
        'points': resolution^3}.  Every later stage works on the mesh and is the same.  With sparse=False the key is absent.
        tsdf=dict(...) takes the surface from rendered views in place of a density level: render_depth from every pose, the depth maps
        fused into a truncated signed distance volume on the same lattice (mesh.TSDFVolume, csrc/mesh_tsdf.hip) and its zero level
        meshed (TSDFVolume.extract: faces whose cell has a corner no view observed are dropped; area-weighted normals).  The surface is
        the one the renders show: no threshold to tune, and haze that never shows in a render leaves no floaters.  Keys: 'poses'
        [N, 3|4, 4], 'intrinsics' (fx, fy, cx, cy), 'H', 'W' (required); 'convention' ('nerfstudio'), 'trunc' (the truncation distance,
        default 4 x the largest lattice step), 'min_opacity' (0.5: below it a pixel is free space), 'carve' (True; False turns
        transparent pixels into "no information" — NaN — in place of "free" — +inf), 'render' (kwargs of render()).  `threshold` and
        `part` play no role (part must be 'all', sparse False); 'threshold' in the result is 0.0, 'volume' the finalised TSDF (positive
        inside), and 'tsdf' joins the dict: {'views', 'trunc', 'observed': share of observed lattice points, 'dropped_faces'}.  Every
        later stage is the same.  With tsdf=None the key is absent.
        fill_holes=True closes the boundary loops the extraction leaves — where the surface leaves the lattice (an aabb tighter than
        the object, an object standing on the box floor), where the TSDF's face rule drops the unobserved side, where component removal
        kept a rim — with mesh.fill_holes (csrc/mesh_holes.hip): every simple loop gets a fan round a new vertex at its centroid (a loop
        of three edges one face); an int >= 3 fills only the loops of at most that many edges.  It runs after component removal and
        before smoothing, clustering and decimation, so the patches are smoothed and decimated with the rest (and belong to the mesh
        'deviation' and bake_from='source' compare with); a fan across a large, non-planar hole is a coarse patch, and loops through a
        pinched vertex stay open.  Not with simplify, whose output need not be manifold; it works with sparse=True and with tsdf=.
        'holes' joins the dict: mesh.fill_holes' info.  topology=True adds 'topology': mesh.topology of the final mesh (edges, boundary
        loops, Euler characteristic, 'watertight', ...).  With the defaults neither key is present.
        color_views=dict(...) takes the colour of color=True and texture=R (one of which it needs) from rendered views in place of one
        field query per point — forward(x, -normal) reads the radiance of a single point in a direction no training ray had, while what
        the renders show is the colour composited along camera rays.  Every pose is rendered with render_view; the surface the
        queried points lie on — the final mesh, or with bake_from='source' the mesh as it stood after marching cubes and component
        removal — is rasterised from the same pose (mesh.rasterize) for the visibility depth, never the field's own depth; and
        mesh.ViewColors (csrc/mesh_view_colors.hip) blends, per point, the views that see it, weighted by cos^power of the viewing
        angle and by the rendered opacity (zero below min_opacity).  Points no view sees fall back to the field query.  Keys: 'poses'
        [N, 3|4, 4], 'intrinsics' (fx, fy, cx, cy), 'H', 'W' (required); 'convention' ('nerfstudio'), 'min_opacity' (0.5), 'render'
        (kwargs of render()), 'depth_tol' (how far a point may lie from the rasterised depth and still count as seen; default twice
        the largest lattice step), 'power' (2) and 'min_cos' (0.2) — documented defaults, not measured optima.  color_views='tsdf'
        reuses the cameras of tsdf= (ValueError without it).  Pinhole views only, and no exposure compensation between views.
        'view_colors' joins the dict: {'views', 'seen': [3] int64 on the device, the points asked (vertices and texels) that 0, 1 and
        >= 2 views saw, 'depth_tol'}.  With color_views=None the key is absent and every output is what it was.
        remesh=R2 (an int) or remesh=dict(resolution=.. | voxel=.., offset=0.0, beta=2.0, probe=2) rebuilds the surface as the zero level
        (with offset: the level `offset`, > 0 thicker, < 0 thinner, in world units) of the mesh's own signed distance on a cubic lattice
        of R2 points along the longest side of its box (mesh.voxel_remesh; the sign is the generalized winding number, csrc/mesh_bvh.hip,
        so the input may have holes, overlapping parts and non-manifold edges).  The output is closed and manifold wherever that level
        set is regular: holes are capped, the faces inside overlapping parts vanish, and detail below a voxel of the new lattice is lost.
        It runs after component removal and fill_holes and before smooth, simplify and target_faces; 'deviation' and bake_from='source'
        compare with the surface as extracted, so they report what the remesh cost, and deviation=True counts it as a lossy pass.
        'remesh' joins the dict: voxel_remesh's info (shape, origin, spacing, bricks, evaluations, rounds, offset, beta).  With
        remesh=None the key is absent and every output is what it was.
        The field's own normals on the vertices: extract_mesh_normals(normals='field', ...), or save_mesh(path, normals='field', ...)."""
        return _export.extract_mesh(
            self, resolution=resolution, threshold=threshold, aabb=aabb, chunk=chunk, part=part, view_dir=view_dir, color=color,
            min_component_faces=min_component_faces, keep_largest=keep_largest, simplify=simplify, target_faces=target_faces, texture=texture,
            smooth=smooth, smooth_lambda=smooth_lambda, smooth_mu=smooth_mu, deviation=deviation, deviation_spacing=deviation_spacing,
            deviation_max_samples=deviation_max_samples, ao=ao, texture_layout=texture_layout, bake_from=bake_from, bake_reach=bake_reach,
            normal_map=normal_map, sparse=sparse, sparse_probe=sparse_probe, tsdf=tsdf, fill_holes=fill_holes, topology=topology,
            color_views=color_views, remesh=remesh)

    @torch.no_grad()
    def extract_mesh_normals(self, normals='field', **kw):
        """extract_mesh(**kw) with the source of the vertex normals chosen (extract_mesh itself keeps the signature its callers know).
        normals='field' replaces the final mesh's vertex normals by the field's own, self.normal(verts) — the analytic gradient of the
        density (csrc/field_normal.hip), which holds sub-voxel orientation that normals interpolated from the lattice cannot — after the
        last geometry stage and before colour, texture and normal-map baking read them.  A vertex keeps its geometric normal where the
        field's is zero or opposes it (dot <= 0); 'field_normals' joins the dict: {'kept_geometric': that count}.  Not with part != 'all',
        tsdf= or remesh=, whose surfaces are not the density's level set (ValueError).  normals='mesh' is extract_mesh(**kw)."""
        args = inspect.signature(NeRFRenderer.extract_mesh).bind(self, **kw)
        args.apply_defaults()
        kw = dict(args.arguments)
        del kw['self']
        return _export.extract_mesh(self, normals=normals, **kw)

    def save_mesh(self, path, **kw):
        """extract_mesh(**kw) written to `path` -> the mesh dict.  A path ending in .obj writes a Wavefront OBJ (mesh.write_obj: positions,
        normals, and with texture=R the UVs, <stem>.mtl and the R x R <stem>.png beside it; vertex colours are not written to OBJ); any other
        .glb a binary glTF 2.0 (mesh.write_glb: one file that holds the welded vertices of mesh.gltf_vertices — positions, normals, UVs,
        tangents — the texture and, with normal_map='tangent', the tangent-space normal map; without texture= the indexed vertices with
        their normals and colours, or the ambient occlusion as grey, as for PLY; unlit unless it carries a normal map); any other
        path a binary PLY (mesh.write_ply: positions, normals, and colours when color=True), which takes no texture.  The cleanup options of
        extract_mesh (min_component_faces, keep_largest, smooth, smooth_lambda, smooth_mu, simplify, target_faces), texture_layout, deviation /
        deviation_spacing, ao, bake_from, bake_reach, sparse, sparse_probe, tsdf, fill_holes, topology, color_views and remesh pass through; normal_map=True writes <stem>_normal.png beside a .obj (a `norm` line
        in the material) and, like texture=, needs an .obj path; normal_map='tangent' needs a .glb path (OBJ carries no tangents) and
        normal_map=True is refused for .glb (glTF has no object-space slot).  A PLY written with ao=K and without color=True carries the ambient occlusion as grey vertex colours
        round(255 ao), so that a viewer shows the cavities of a geometry-only export; with color=True the field's colours are written
        unchanged (a NeRF's radiance already contains its shading, so AO is never multiplied into baked colour or texture)."""
        return _export.save_mesh(self, path, **kw)

    def render_mesh(self, mesh, c2w, intrinsics, H, W, path=None, map='texture', **kw):
        """Preview of an exported mesh from a camera pose, rasterised on the device (mesh.render_mesh, csrc/mesh_raster.hip).  `mesh` is the
        dict extract_mesh / save_mesh return: its verts, faces, normals, colors, uvs and texture are forwarded (so the texture is shown
        when the mesh has one, else the vertex colours, else the normals); the camera is generate_rays' (c2w [3, 4] or [4, 4], intrinsics
        (fx, fy, cx, cy), convention= in **kw).  map='normal_map' shows the mesh's normal map (extract_mesh(normal_map=True or 'tangent'), whichever it holds) in place of
        its texture, through the same 'texture' shading.  With `path` the image is also written as a PNG (mesh.write_png).
        -> (image [H, W, 3] uint8, mask [H, W] bool, the visibility dict of mesh.rasterize)."""
        if map not in ('texture', 'normal_map'):
            raise ValueError(f"render_mesh: map must be 'texture' or 'normal_map', got {map!r}")
        if map == 'normal_map' and mesh.get('normal_map') is None:
            raise ValueError("render_mesh: map='normal_map' needs a mesh from extract_mesh(normal_map=True)")
        image, mask, vis = _mesh.render_mesh(mesh['verts'], mesh['faces'], c2w, intrinsics, H, W, normals=mesh.get('normals'),
                                             colors=mesh.get('colors'), uvs=mesh.get('uvs'), texture=mesh.get(map), **kw)
        if path is not None:
            _mesh.write_png(path, image)
        return image, mask, vis

    @torch.no_grad()
    def render_depth(self, c2w, intrinsics, H, W, convention='nerfstudio', min_opacity=0.5, max_ray_batch=1 << 16, **render_kw):
        """Depth map of one pinhole view (the camera of provider_utils.generate_rays and mesh.rasterize: c2w [3, 4] or [4, 4], intrinsics
        (fx, fy, cx, cy)), rendered through render(..., staged=True, perturb=False, **render_kw) in batches of max_ray_batch rays.
        -> {'depth': [H, W] float32, 'opacity': [H, W] float32}.  depth is the METRIC DISTANCE ALONG THE RAY of the expected termination,
        sum(w t) / sum(w), whichever path rendered it; pixels whose opacity sum(w) is below min_opacity get +inf (nothing was hit), which
        is what mesh.TSDFVolume.integrate(depth_kind='ray') reads as free space.  The two paths return different things under 'depth':
        run_cuda sum(w t), and run() sum(w clamp((t - near) / (far - near), 0, 1)) as the reference does (nerf/renderer.py:435-436), so
        the latter is mapped back with the ray's own near / far (near_far_from_aabb with the box and min_near that run() used)."""
        return _export.render_view(self, c2w, intrinsics, H, W, convention, min_opacity, max_ray_batch, render_kw, False, "render_depth")

    @torch.no_grad()
    def render_view(self, c2w, intrinsics, H, W, convention='nerfstudio', min_opacity=0.5, max_ray_batch=1 << 16, **render_kw):
        """render_depth's view with its colour, from the same one pass per ray batch: -> {'image': [H, W, 3] float32, the composited
        colour render() returns (over its background, where one is set), 'depth', 'opacity'}; depth and opacity are render_depth's, bit
        for bit.  What extract_mesh(color_views=...) projects onto the mesh.
        Five keywords are taken out of **render_kw (defaults normals=False, shading=None, light_d=None, ambient_ratio=0.1, path=None):
        normals=True (run() only: the occupancy march raises NotImplementedError) adds 'normal' [H, W, 3]: the world-space normal map
        run(normals=True) composites, renormalised per pixel, zero where the opacity is below min_opacity.
        shading in ('normal', 'lambertian', 'textureless') implies normals and adds 'shaded' [H, W, 3]: 'normal' (n + 1) / 2;
        'lambertian' image * (a + (1 - a) max(0, n . l)) with a = ambient_ratio and l = light_d normalised (default: towards the camera,
        against the view direction of the image centre); 'textureless' the same with albedo 1.  This is DEFERRED shading of the
        composited normal, one evaluation per pixel — not the per-sample shading of stable-dreamfusion, which lights every sample before
        compositing.  `path` writes 'shaded' (without shading: the normal map as (n + 1) / 2, without normals: the image) as a PNG
        (mesh.write_png).  With the defaults the result is what it was."""
        own = {k: render_kw.pop(k, v) for k, v in _export.VIEW_OPTIONS.items()}
        return _export.render_view(self, c2w, intrinsics, H, W, convention, min_opacity, max_ray_batch, render_kw, True, "render_view", **own)

    def render(self, rays_o, rays_d, staged=False, max_ray_batch=2048, **kwargs):
        """renderer.py:1719-1733."""
        _run = self.run_cuda if self.cuda_ray else self.run
        return _run(rays_o, rays_d, **kwargs)
