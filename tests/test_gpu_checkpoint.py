"""GPU: the training state that crosses a checkpoint file.  A trainer that saves (`save_checkpoint(full=True)`), is rebuilt from nothing and loads
(`load_checkpoint`) must go on exactly where the uninterrupted run goes: the float32 parameters, the Adam moments and step count, the loss scaler's
device state (whose count of applied steps drives the bias correction inside the Adam kernels), the fp16 shadow of the grid table, the packed
weight images, the learning-rate decay (a function of `global_step`), the occupancy grid of the march path, the per-view hipGraphs of a live
trainer.  (a) resume, (b) roll-back inside a live graphed trainer and (d) `--editing_from` demand bit equality; (c) pins the saved state dicts and
cross-loading against torch.optim.Adam + GradScaler at the tolerance of test_dynamic_loss_scaler_matches_torch_gradscaler.

Shape of (a), (b): 8 levels, 2^15-entry table, 64 x 64 rays x 64 samples = 2^21 (sample, level) pairs per backward — above the 2^20 at which the
grid backward takes the order-independent binned scatter (below it the float-atomic kernel runs, which is not reproducible run to run), so bit
equality is a fair demand; every case checks first that the uninterrupted run alone repeats bit for bit.

The march path samples only the occupied cells: a 64 x 64 view gives 66.8 k samples, 2^19 pairs — the float-atomic kernel, and the uninterrupted
run did not repeat (measured: none of three repeats).  Its case takes 128 x 128 views: 266 k to 612 k samples per step, 2^21 pairs and more, and
the run repeats.

The float32 trainer is the other exception.  Its scatter records are float32 and are summed with float atomics (the parity path: csrc/gridencoder_binned.hip
keeps ds_add_f32 for them, and below 2^20 pairs the plain atomic kernel runs), so an fp32 run does not repeat at the shape above, nor at any shape
where two waves add into one table entry: five runs of ten steps each differed from the first at 64 x 64 x (32 + 32) and at 16 x 16 x (8 + 8), one
of four did at 4 x 4 x (3 + 2) (80 samples: two waves per level), none at 2 x 2 x (3 + 2) and 1 x 1 x (3 + 2).  With 2 x 2 rays x 5 samples the 20
samples of a level are lanes of ONE wave, whose atomics on one address retire in lane order — so that is the shape of the f32 case: the largest
at which its uninterrupted run is reproducible.  What the case is there for does not depend on the size: the static loss scale, Adam's step taken
from the host-side counter the file restores, float32 moments, the learning-rate decay.

Measured on an MI355X, seconds per case: resume f16-dynamic 2.1 (the process's first steps: workspaces, first launches), unfused table 0.04, f32 0.05,
march 0.14; roll-back 0.06; state dicts 0.07; cross-loading 0.01 each; static scale < 0.005; editing_from 1.3 (run) and 1.2 (march)."""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # sibling test modules' helpers

N, K = 6, 4                     # steps before the save, steps after
SEED_AFTER = 4321               # torch.manual_seed right after step N (run A) / right after the load (run B)
SKIP_AT = 2                     # the step (0-based, < N) whose target has one inf pixel: the loss scaler skips it
CENTRE = 32 * 64 + 32           # ... the centre pixel of a 64 x 64 view
MARCH_HW = 128                  # the march case's view size (see the module docstring); its inf pixel is the centre too: that ray crosses occupied cells
GRID = dict(num_levels=8, log2_hashmap_size=15, desired_resolution=256)
KW = dict(num_steps=32, upsample_steps=32)
INF = float('inf')


@pytest.fixture(autouse=True)
def _restore_default_dtype():
    from customnerf_amd import tcnn
    yield
    tcnn.set_default_dtype(torch.float32)               # the fp16 default must not leak into later tests


F32_HW, F32_KW = 2, dict(num_steps=3, upsample_steps=2)          # the float32 case's shape: see the module docstring
HW = {'f32': F32_HW, 'f16-march': MARCH_HW}                      # every other case: 64


@functools.lru_cache(maxsize=None)
def _scene(hw=64):
    """two hw x hw views (o, d, rgb, mask), made once and never written"""
    from test_gpu_train import _target_scene
    return _target_scene(hw, hw, 2)


def _recon(case, seed=0):
    from customnerf_amd import scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.trainer import ReconTrainer
    fp16 = case != 'f32'
    tcnn.set_default_dtype(torch.float16 if fp16 else torch.float32)
    torch.manual_seed(seed)
    opt = sc.make_opt(fp16=fp16, cuda_ray=(case == 'f16-march'), lr=5e-3, iters=40, **GRID)     # (iters 40: the decay moves the rate 6 % per step)
    if case == 'f16-dynamic-unfused-table':
        opt.fuse_table_adam = False
    model = NeRFNetwork(opt).cuda()
    return ReconTrainer(model, opt, fp16=fp16), model


def _refresh_occupancy(tr, model):
    with torch.autocast('cuda', dtype=torch.float16, enabled=tr.fp16):
        model.update_extra_state()


def _step(tr, i, case, skip=False):
    hw = HW.get(case, 64)
    o, d, rgb, mask = _scene(hw)
    v = i % 2
    target = rgb[v]
    if skip:
        target = rgb[v].clone()
        target[hw // 2 * hw + hw // 2, 0] = INF                           # an inf value in a loss target: a non-finite gradient, which the scaler answers by skipping
    kw = dict(dt_gamma=0, max_steps=1024) if case == 'f16-march' else F32_KW if case == 'f32' else KW
    loss, _ = tr.train_step(o[v], d[v], target, mask[v], **kw)
    return float(loss)


def _state(tr, model, march=False):
    """everything that must survive the file, cloned"""
    sd = tr.optimizer.state_dict()
    ps = [p for g in tr.optimizer.param_groups for p in g['params']]
    st = dict(params=[p.detach().clone() for p in ps],
              exp_avg=[tr.optimizer.state[p]['exp_avg'].clone() for p in ps],
              exp_avg_sq=[tr.optimizer.state[p]['exp_avg_sq'].clone() for p in ps],
              steps=[int(sd['state'][i]['step']) for i in range(len(ps))],
              scaler=tr.scaler.state.clone() if tr.scaler is not None else None,
              global_step=tr.global_step, lrs=[g['lr'] for g in tr.optimizer.param_groups])
    enc = model.pos_en
    if tr.fp16:
        sh = tr.optimizer.half_shadows.get(enc.embeddings)
        assert sh is not None and sh.data_ptr() == enc.half_table().data_ptr()      # the shadow Adam writes is the one the gather reads
        assert torch.equal(enc.half_table(), enc.embeddings.detach().half())
        st['half'] = enc.half_table().clone()
    if march:
        st.update(density_grid=model.density_grid.clone(), density_bitfield=model.density_bitfield.clone(), mean_count=model.mean_count,
                  mean_density=model.mean_density)
    return st


def _assert_same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            assert torch.equal(x, y), k
        elif isinstance(x, list) and x and torch.is_tensor(x[0]):
            assert len(x) == len(y)
            for i, (xx, yy) in enumerate(zip(x, y)):
                assert torch.equal(xx, yy), (k, i)
        else:
            assert x == y, (k, x, y)


# ------------------------------------------------------------------------------------------------ (a) resume is bit-identical
@pytest.mark.parametrize("case", ["f16-dynamic", "f16-dynamic-unfused-table", "f32", "f16-march"])
def test_resume_from_a_full_checkpoint_is_bit_identical(case, tmp_path):
    """N steps (one of them skipped by the loss scaler) + save + a NEW model (built under another seed) and trainer + load + K steps == N + K steps.
    Compared with torch.equal / ==: the K losses, every parameter, exp_avg and exp_avg_sq, the Adam step counts (as saved: the applied steps), the
    scaler's device state, the fp16 shadow (against embeddings.half() too), global_step, the learning rates after the last step; on the march path
    also density_grid, density_bitfield, mean_count, mean_density."""
    march = case == 'f16-march'

    def first_n():
        tr, model = _recon(case)
        if march:
            _refresh_occupancy(tr, model)
        for i in range(N):
            _step(tr, i, case, skip=(i == SKIP_AT and tr.scaler is not None))
        if march:
            _refresh_occupancy(tr, model)
        if tr.scaler is not None:
            assert tr.scaler.good_steps() == N - 1       # the skip happened, and no other
        return tr, model

    def run_a():
        tr, model = first_n()
        torch.manual_seed(SEED_AFTER)
        losses = [_step(tr, i, case) for i in range(N, N + K)]
        return losses, _state(tr, model, march)

    def run_b():
        tr, model = first_n()
        path = tr.save_checkpoint(str(tmp_path / "df_ep0001.pth"), epoch=1, full=True)
        del tr, model
        tr2, model2 = _recon(case, seed=99)
        info = tr2.load_checkpoint(path)
        assert info['global_step'] == N and info['epoch'] == 1 and info['missing_keys'] == [] and info['unexpected_keys'] == []
        assert tr2.global_step == N
        torch.manual_seed(SEED_AFTER)
        losses = [_step(tr2, i, case) for i in range(N, N + K)]
        return losses, _state(tr2, model2, march)

    la, sa = run_a()
    la2, sa2 = run_a()
    assert all(np.isfinite(la)), la
    assert la == la2                                     # precondition: the uninterrupted run repeats bit for bit at this shape
    _assert_same(sa, sa2)
    lb, sb = run_b()
    assert lb == la, (la, lb)
    _assert_same(sa, sb)
    assert sa['global_step'] == N + K and sa['steps'] == [N + K - (0 if sa['scaler'] is None else 1)] * 4


# ------------------------------------------------------------------------------------------------ (b) rolling back inside a live trainer
def test_rolling_a_live_graphed_trainer_back_is_bit_identical(tmp_path):
    """N graphed steps on two alternating views (graphs exist), save, three more steps (one skipped: the scale moves), load_checkpoint on the SAME
    trainer, K steps == the uninterrupted N + K graphed steps.  Finds a stale half shadow, stale packed weights, a stale graph, optimiser tensors
    something still points at.  (A view's first visit takes two eager steps and the captured one: `global_step` is the calls + 4.)"""
    def run(rollback):
        tr, model = _recon('f16-dynamic')
        views = [tuple(t[v].clone() for t in _scene()) for v in range(2)]          # resident tensors of this run's own: one of them is written below

        def call(i, skip=False):
            o, d, rgb, mask = views[i % 2]
            if skip:
                keep = rgb[CENTRE, 0].clone()
                rgb[CENTRE, 0] = INF
            loss, _ = tr.train_step_graphed(o, d, rgb, mask, **KW)
            loss = float(loss)
            if skip:
                rgb[CENTRE, 0] = keep
            return loss

        for i in range(N):
            call(i, skip=(i == 3))                                                 # (a replay: both views were captured by then)
        assert len(tr._graphs) == 2 and tr.global_step == N + 4 and tr.scaler.good_steps() == N + 3
        if rollback:
            graphs = [e[0] for e in tr._graphs.values()]
            scale = tr.scaler.get_scale()
            path = tr.save_checkpoint(str(tmp_path / "live.pth"), full=True)
            for i in range(N, N + 3):
                call(i, skip=(i == N + 1))
            assert tr.scaler.get_scale() == 0.5 * scale and tr.global_step == N + 7
            tr.load_checkpoint(path)
            assert tr.global_step == N + 4 and tr.scaler.get_scale() == scale
            assert [e[0] for e in tr._graphs.values()] == graphs                  # nothing a graph references moved: they are kept, and replayed below
        torch.manual_seed(SEED_AFTER)
        losses = [call(i) for i in range(N, N + K)]
        return losses, _state(tr, model)

    la, sa = run(False)
    la2, sa2 = run(False)
    assert all(np.isfinite(la)) and la == la2
    _assert_same(sa, sa2)
    lb, sb = run(True)
    assert lb == la, (la, lb)
    _assert_same(sa, sb)
    assert sa['steps'] == [N + K + 3] * 4 and sa['global_step'] == N + K + 4


# ------------------------------------------------------------------------------------------------ (c) step counts, cross-loading against torch
class _Holder(torch.nn.Module):
    """the `model` of a checkpoint for a bare list of parameters"""

    def __init__(self, params):
        super().__init__()
        self.p = torch.nn.ParameterList(params)


SHAPES = [(70001,), (37, 16), (8,)]         # one tensor takes the per-tensor launch, two the multi-tensor launch (which also applies update())
TOL = dict(atol=1e-6, rtol=1e-5)            # test_dynamic_loss_scaler_matches_torch_gradscaler's, for parameters


def _grad_sequence(n, bad):
    g = torch.Generator(device="cuda").manual_seed(1)
    seq = []
    for step in range(n):
        grads = [torch.randn(s, device="cuda", generator=g) for s in SHAPES]
        if step in bad:
            grads[step % 3].view(-1)[5] = bad[step]
        seq.append(grads)
    return seq


def _torch_pair(params, scaler=True):
    opt = torch.optim.Adam([{'params': params[:1], 'lr': 1e-2}, {'params': params[1:], 'lr': 1e-3}], betas=(0.9, 0.99), eps=1e-15)
    return opt, (torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=4) if scaler else None)


def _our_pair(params, scaler=True):
    from customnerf_amd.optim import DynamicLossScaler, FusedAdam
    from customnerf_amd.trainer import flat_grad_buffer
    opt = FusedAdam([{'params': params[:1], 'lr': 1e-2}, {'params': params[1:], 'lr': 1e-3}], betas=(0.9, 0.99), eps=1e-15)
    opt.scaler = DynamicLossScaler("cuda", init_scale=1024.0, growth_interval=4) if scaler else None
    opt._test_flat = flat_grad_buffer(params)
    return opt, opt.scaler


def _torch_steps(params, opt, scaler, seq):
    """-> per step (scale before the step, was it skipped)"""
    scaler.scale(torch.zeros(1, device="cuda"))                     # GradScaler creates its device state lazily (from what load_state_dict left)
    trace = []
    for grads in seq:
        s = scaler.get_scale()
        before = [p.detach().clone() for p in params]
        for p, g in zip(params, grads):
            p.grad = g * s                                            # what backward of the scaled loss leaves behind
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()
        trace.append((s, all(torch.equal(a, b) for a, b in zip(before, params))))
    return trace


def _our_steps(params, opt, scaler, seq, static_scale=None):
    from customnerf_amd.trainer import check_grads_finite
    trace = []
    for grads in seq:
        s = scaler.get_scale() if scaler is not None else static_scale
        before = [p.detach().clone() for p in params]
        for q, g in zip(params, grads):
            q.grad.copy_(g * s)
        if scaler is not None:
            check_grads_finite(scaler, params, opt._test_flat)
        else:
            opt.grad_scale_inv = 1.0 / s
        opt.step()
        if scaler is not None:
            scaler.update()
        trace.append((s, all(torch.equal(a, b) for a, b in zip(before, params))))
    return trace


@functools.lru_cache(maxsize=None)
def _six_steps():
    """FusedAdam + DynamicLossScaler and torch.optim.Adam + GradScaler side by side on one recorded gradient sequence: two parameter groups,
    growth_interval 4, step 3 of 6 non-finite; then both saved (checkpoint.checkpoint_state, deep-copied: state_dict() hands out the live tensors),
    and the torch pair taken four steps further without a break (step 8 non-finite).  Computed once, shared, never written afterwards.
    (Steps 4-6 are three clean steps in a row, so the growth tracker crosses the save at 3 and the growth lands on the first step after it: a loader
    that drops `_growth_tracker`, or a scaler that forgets it, shows in the scale.)"""
    from customnerf_amd import checkpoint as ck
    torch.manual_seed(0)
    init = [torch.randn(s, device="cuda") for s in SHAPES]
    seq = _grad_sequence(10, {2: INF, 7: float('nan')})
    p_ref, p_our = [[torch.nn.Parameter(p.clone()) for p in init] for _ in range(2)]
    opt_ref, sc_ref = _torch_pair(p_ref)
    opt_our, sc_our = _our_pair(p_our)
    trace_ref = _torch_steps(p_ref, opt_ref, sc_ref, seq[:6])
    trace_our = _our_steps(p_our, opt_our, sc_our, seq[:6])
    out = dict(init=init, seq=seq, trace_ref=trace_ref, trace_our=trace_our, params_ref=[p.detach().clone() for p in p_ref],
               params_our=[p.detach().clone() for p in p_our],
               sd_ref=copy.deepcopy(opt_ref.state_dict()), sd_our=copy.deepcopy(opt_our.state_dict()),
               ss_ref=sc_ref.state_dict(), ss_our=sc_our.state_dict(),
               file_ref=copy.deepcopy(ck.checkpoint_state(_Holder(p_ref), global_step=6, optimizer=opt_ref, scaler=sc_ref, full=True)),
               file_our=copy.deepcopy(ck.checkpoint_state(_Holder(p_our), global_step=6, optimizer=opt_our, scaler=sc_our, full=True)))
    out['trace_cont'] = _torch_steps(p_ref, opt_ref, sc_ref, seq[6:])
    out['params_cont'] = [p.detach().clone() for p in p_ref]
    return out


def _resume(file, ours):
    """fresh parameters (other values), optimiser and scaler of the wanted kind; load `file` through checkpoint.load_checkpoint; steps 7-10.
    -> per step ((scale before it, skipped?), parameters after it), Adam's saved step after step 10, the scaler's state dict"""
    from customnerf_amd import checkpoint as ck
    s = _six_steps()
    params = [torch.nn.Parameter(torch.randn_like(p)) for p in s['init']]
    opt, sc = (_our_pair if ours else _torch_pair)(params)
    info = ck.load_checkpoint(_Holder(params), copy.deepcopy(file), optimizer=opt, scaler=sc, log=lambda m: pytest.fail(m))
    assert info['global_step'] == 6
    per_step = []
    for grads in s['seq'][6:]:
        per_step.append(((_our_steps if ours else _torch_steps)(params, opt, sc, [grads])[0], [p.detach().clone() for p in params]))
    return per_step, int(opt.state_dict()['state'][0]['step']), sc.state_dict()


@functools.lru_cache(maxsize=None)
def _torch_to_torch():
    return _resume(_six_steps()['file_ref'], ours=False)


def test_saved_optimizer_and_scaler_state_match_torch_key_by_key():
    """At step 6 (one of them skipped) FusedAdam.state_dict() against torch.optim.Adam.state_dict() and DynamicLossScaler.state_dict() against
    GradScaler.state_dict(): Adam's `step` equal as integers — 5, the applied steps, not the 6 calls of step() —, scale and _growth_tracker equal,
    the moments within the parameter tolerance of test_dynamic_loss_scaler_matches_torch_gradscaler (atol 1e-6, rtol 1e-5; measured: 2.4e-07 for exp_avg, 2.7e-07 for exp_avg_sq at most)."""
    s = _six_steps()
    assert s['trace_our'] == s['trace_ref'] and [skipped for _, skipped in s['trace_ref']] == [False, False, True, False, False, False]
    for p, q in zip(s['params_ref'], s['params_our']):
        assert torch.allclose(p, q, **TOL)
    sd_ref, sd_our = s['sd_ref'], s['sd_our']
    assert set(sd_our) == set(sd_ref) and set(sd_our['state']) == set(sd_ref['state']) == {0, 1, 2}
    for i in range(3):
        a, b = sd_our['state'][i], sd_ref['state'][i]
        assert set(a) == set(b) == {'step', 'exp_avg', 'exp_avg_sq'}
        assert type(a['step']) is int and a['step'] == int(b['step']) == 5
        for k in ('exp_avg', 'exp_avg_sq'):
            print(f"step 6, tensor {i}, {k}: max |ours - torch| {float((a[k] - b[k]).abs().max()):.3e}")
            assert torch.allclose(a[k], b[k], **TOL), (i, k)
    for ga, gb in zip(sd_our['param_groups'], sd_ref['param_groups']):
        # (torch.optim.Adam fills in its remaining defaults itself when it loads a group, but reads these without one)
        assert set(ga) <= set(gb) and {'lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'params'} <= set(ga)
        for k in ga:
            assert ga[k] == gb[k], k
    ss_ref, ss_our = s['ss_ref'], s['ss_our']
    assert set(ss_our) - set(ss_ref) == {'_good_steps'} and ss_our['_good_steps'] == 5
    for k, v in ss_ref.items():
        assert ss_our[k] == v and type(ss_our[k]) is type(v), k
    assert ss_ref['_growth_tracker'] == 3 and ss_ref['scale'] == 512.0


@pytest.mark.parametrize("combo", ["torch-to-ours", "ours-to-ours", "ours-to-torch"])
def test_cross_loading_follows_the_torch_trajectory(combo):
    """Steps 7-10 (step 8 non-finite) after loading the step-6 file through checkpoint.load_checkpoint, against torch -> torch: the parameters at
    atol 1e-6 / rtol 1e-5 after every step, the scale before every step, the skipped steps and Adam's final step (8) exactly.  torch -> ours: the
    reference's 'scaler' entry has no count of applied steps and Adam's `step` is a 0-dim tensor; ours -> torch: torch.optim.Adam reads the step
    this package wrote.  (The file itself costs nothing: torch -> torch against the torch pair that never stopped is measured below — 0.)"""
    s = _six_steps()
    want, want_step, want_sc = _torch_to_torch()
    assert [t for t, _ in want] == [(512.0, False), (1024.0, True), (512.0, False), (512.0, False)] and want_step == 8
    assert s['trace_cont'] == [t for t, _ in want]
    d_file = max(float((p - q).abs().max()) for p, q in zip(s['params_cont'], want[-1][1]))
    print(f"uninterrupted torch vs torch -> torch after step 10: max |diff| {d_file:.3e}")
    got, got_step, got_sc = _resume(s['file_ref'] if combo.startswith("torch") else s['file_our'], ours=combo.endswith("ours"))
    assert [t for t, _ in got] == [t for t, _ in want]                         # the scale before every step and which steps were skipped: exactly
    assert got_sc['scale'] == want_sc['scale'] and got_sc['_growth_tracker'] == want_sc['_growth_tracker']
    for n, ((_, pg), (_, pw)) in enumerate(zip(got, want)):
        for i, (a, b) in enumerate(zip(pg, pw)):
            if n == 3:
                print(f"{combo}, step 10, tensor {i}: max |diff to torch -> torch| {float((a - b).abs().max()):.3e}")
            assert torch.allclose(a, b, **TOL), (combo, 7 + n, i, float((a - b).abs().max()))
    assert got_step == want_step


def test_torch_adam_state_resumes_under_a_static_loss_scale():
    """torch -> ours without a scaler object (a float32 or static-scale trainer): the kernel takes Adam's step from the host-side counter, which
    the file restores — from a 0-dim tensor — as an int"""
    from customnerf_amd import checkpoint as ck
    init = _six_steps()['init']
    clean = _grad_sequence(10, {})
    p_t = [torch.nn.Parameter(p.clone()) for p in init]
    opt_t, _ = _torch_pair(p_t, scaler=False)
    for grads in clean[:6]:
        for p, g in zip(p_t, grads):
            p.grad = g.clone()
        opt_t.step()
    file_t = copy.deepcopy(ck.checkpoint_state(_Holder(p_t), global_step=6, optimizer=opt_t, full=True))
    assert 'scaler' not in file_t
    p_s = [torch.nn.Parameter(torch.randn_like(p)) for p in init]
    opt_s, _ = _our_pair(p_s, scaler=False)
    ck.load_checkpoint(_Holder(p_s), file_t, optimizer=opt_s, log=lambda m: pytest.fail(m))
    assert all(int(opt_s.state[p]['step']) == 6 for p in p_s)
    for n, grads in enumerate(clean[6:]):
        for p, g in zip(p_t, grads):
            p.grad = g.clone()
        opt_t.step()
        _our_steps(p_s, opt_s, None, [grads], static_scale=128.0)
        for i, (a, b) in enumerate(zip(p_s, p_t)):
            assert torch.allclose(a, b, **TOL), ("static", 7 + n, i, float((a - b).abs().max()))
    assert opt_s.state_dict()['state'][0]['step'] == int(opt_t.state_dict()['state'][0]['step']) == 10


# ------------------------------------------------------------------------------------------------ (d) --editing_from
@pytest.mark.parametrize("march", [False, True], ids=["run", "march"])
def test_editing_from_a_saved_reconstruction(march, tmp_path):
    """A reconstruction trained for N steps and saved with full=False, loaded with model_only=True into fresh networks — the edited field and the
    frozen pretrained one of an EditTrainer — against the source still in memory: an unperturbed render() bit for bit in fp16 and in fp32
    compute dtype (march: through the restored occupancy bitfield), EditTrainer.get_pt of the loaded pretrained field, and the parameters after
    one EditTrainer.train_step on the loaded pair against the in-memory pair.  (The editing step renders through run(): a checkpoint of the march
    path brings its occupancy buffers as unexpected keys, which the edit networks — like the reference's strict=False load — pass over.)"""
    from customnerf_amd import checkpoint as ck, scene as sc, tcnn
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.sd.editing import EditTrainer
    from customnerf_amd.trainer import ReconTrainer
    from test_gpu_sd_editing import _setup
    edit_kw = dict(keep_bg=1000.0, lambda_sd=0.01)
    o, d, rgb, mask = _scene()

    # ---- the source: _setup's field geometry, trained as a reconstruction
    tcnn.set_default_dtype(torch.float16)
    torch.manual_seed(5)
    opt_src = sc.make_opt(fp16=True, num_levels=8, num_steps=16, upsample_steps=16, cfg=7.5, log_loss_item=False, cuda_ray=march, lr=5e-3, iters=40, **edit_kw)
    source = NeRFNetwork(opt_src).cuda()
    tr_src = ReconTrainer(source, opt_src, fp16=True)
    if march:
        _refresh_occupancy(tr_src, source)
    kw = dict(dt_gamma=0, max_steps=1024) if march else dict(num_steps=16, upsample_steps=16)
    for i in range(N):
        tr_src.train_step(o[i % 2], d[i % 2], rgb[i % 2], mask[i % 2], **kw)
    if march:
        _refresh_occupancy(tr_src, source)
        assert int(source.density_bitfield.sum()) > 0 and source.mean_count > 0
    assert tr_src.scaler.good_steps() > 0
    path = tr_src.save_checkpoint(str(tmp_path / "df_ep0001.pth"), epoch=1, full=False)
    assert 'optimizer' not in torch.load(path, weights_only=False)

    # ---- an unperturbed render of a fresh network loaded from the file, in both compute dtypes
    def render(m, half):
        m.eval()
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16, enabled=half):
            out = m.render(o[1], d[1], staged=True, perturb=False, force_all_rays=True, num_steps=16, upsample_steps=16, dt_gamma=0, max_steps=1024)
        return [out[k].float().clone() for k in ('image', 'depth', 'weights_sum')]

    for half in (True, False):
        tcnn.set_default_dtype(torch.float16 if half else torch.float32)
        torch.manual_seed(11)
        loaded = NeRFNetwork(opt_src).cuda()
        info = ck.load_checkpoint(loaded, path, model_only=True, map_location="cuda")
        assert info['missing_keys'] == [] and info['unexpected_keys'] == [] and info['global_step'] is None
        if half:
            mem = source
        else:                                                            # the compute dtype is fixed at construction: the source's state in a float32 twin
            mem = NeRFNetwork(opt_src).cuda()
            mem.load_state_dict(source.state_dict())
            mem.pos_en.invalidate_half_table()
            if march:
                mem.mean_count, mem.mean_density = source.mean_count, source.mean_density
        assert loaded._half() == mem._half() == half
        if march:
            assert loaded.mean_count == source.mean_count and loaded.mean_density == source.mean_density
            assert torch.equal(loaded.density_bitfield, source.density_bitfield) and torch.equal(loaded.density_grid, source.density_grid)
        for a, b in zip(render(loaded, half), render(mem, half)):
            assert torch.isfinite(a).all() and torch.equal(a, b)
    source.train()

    # ---- the editing trainer on the loaded pair and on the in-memory pair
    def in_memory(like):
        if not march:
            return copy.deepcopy(source)
        m = copy.deepcopy(like)                                         # (a run()-path network with the source's parameters)
        with torch.no_grad():
            for p, q in zip(m.parameters(), source.parameters()):
                p.copy_(q)
        m.pos_en.invalidate_half_table()
        return m

    tr_l, model_l, pre_l, data = _setup(res=64, **edit_kw)
    occupancy = ['density_grid', 'density_bitfield', 'step_counter'] if march else []
    info = tr_l.load_checkpoint(path, model_only=True)
    assert info['missing_keys'] == [] and info['unexpected_keys'] == occupancy and tr_l.global_step == 0
    ck.load_checkpoint(pre_l, path, model_only=True, map_location="cuda", log=lambda *_: None)
    tr_m0, model_m0, _, _ = _setup(res=64, **edit_kw)                   # (a second guidance with the same weights, for the in-memory pair)
    model_m, pre_m = in_memory(model_m0).train(), in_memory(model_m0).eval()
    tr_m = EditTrainer(model_m, pre_m, tr_m0.guidance, tr_m0.opt, tr_m0.text_z, tr_m0.text_z_fg)
    for a, b in zip(model_l.parameters(), model_m.parameters()):
        assert torch.equal(a, b)
    rgbs, msk, rays_o, rays_d, H, W, _ = data(0)
    pts = []
    for tr in (tr_l, tr_m):
        torch.manual_seed(21)
        pts.append(tr.get_pt(rays_o, rays_d, "probe", None, 1, H, W))
        tr.pt_dict.clear()
    for a, b in zip(pts[0][:4], pts[1][:4]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    after = []
    for tr, m in ((tr_l, model_l), (tr_m, model_m)):
        torch.manual_seed(22)
        loss, _ = tr.train_step(data(0))
        after.append((float(loss), [p.detach().clone() for p in m.parameters()], tr.scaler.state.clone()))
    assert np.isfinite(after[0][0]) and after[0][0] == after[1][0]
    assert torch.equal(after[0][2], after[1][2])
    for a, b, c in zip(after[0][1], after[1][1], source.parameters()):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, c) for a, c in zip(after[0][1], source.parameters()))      # the step moved something
    assert torch.equal(model_l.pos_en.half_table(), model_l.pos_en.embeddings.detach().half())
