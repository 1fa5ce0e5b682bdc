"""CPU: checkpoint files in the reference trainer's format (utils_init_nerf.py:779-901) round-trip through customnerf_amd.checkpoint."""
import torch
import pytest


def _model(**kw):
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.scene import make_opt
    return NeRFNetwork(make_opt(num_levels=4, **kw))


def test_checkpoint_roundtrip_and_reference_structure(tmp_path):
    from customnerf_amd import checkpoint as ck
    m = _model(cuda_ray=True)
    with torch.no_grad():
        for p in m.parameters():
            p.uniform_(-1, 1)
        m.density_grid.uniform_(0, 20)
    m.mean_count, m.mean_density = 123, 4.5
    opt = torch.optim.Adam(m.get_params(1e-3), betas=(0.9, 0.99), eps=1e-15)
    path = ck.save_checkpoint(str(tmp_path / "checkpoints" / "df_ep0007.pth"), m, epoch=7, global_step=700, optimizer=opt, full=True)
    raw = torch.load(path, weights_only=False)
    assert set(raw) == {'epoch', 'global_step', 'stats', 'mean_count', 'mean_density', 'optimizer', 'model'}        # utils_init_nerf.py:784-799
    for k in ("aabb_train", "aabb_infer", "pos_en.embeddings", "pos_en.offsets", "network.params", "density_network.params", "rgb_network.params",
              "density_grid", "density_bitfield", "step_counter"):
        assert k in raw['model'], k
    m2 = _model(cuda_ray=True)
    opt2 = torch.optim.Adam(m2.get_params(1e-3), betas=(0.9, 0.99), eps=1e-15)
    info = ck.load_checkpoint(m2, path, optimizer=opt2)
    assert info['epoch'] == 7 and info['global_step'] == 700 and info['missing_keys'] == [] and info['unexpected_keys'] == []
    assert m2.mean_count == 123 and m2.mean_density == 4.5
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    assert ck.latest_checkpoint(str(tmp_path / "checkpoints")) == path


def test_checkpoint_reference_style_inputs(tmp_path):
    from customnerf_amd import checkpoint as ck
    m = _model()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["pos_en.embeddings"] = torch.full_like(sd["pos_en.embeddings"], 0.25)
    # bare state dict (:850-853)
    info = ck.load_checkpoint(_model(), sd)
    assert info['epoch'] is None
    # model_only + unexpected / missing keys are reported, not fatal (strict=False, :855-860)
    ref = {'epoch': 3, 'global_step': 30, 'stats': {}, 'model': dict(sd, **{"bg_net.params": torch.zeros(4)})}
    del ref['model']['rgb_network.params']
    m3 = _model()
    info = ck.load_checkpoint(m3, ref, model_only=True, log=lambda *_: None)
    assert info['unexpected_keys'] == ["bg_net.params"] and info['missing_keys'] == ["rgb_network.params"] and info['epoch'] is None
    assert float(m3.pos_en.embeddings.detach().mean()) == 0.25
    # a table of another geometry is refused with a clear message
    bad = {'model': dict(sd, **{"pos_en.embeddings": torch.zeros(10, 2)})}
    with pytest.raises(ValueError):
        ck.load_checkpoint(_model(), bad)


def test_full_checkpoint_carries_lr_scheduler_and_ema(tmp_path):
    """the optional entries of the reference's `full` checkpoint (utils_init_nerf.py:794-800) and their restore (:862-894)"""
    from customnerf_amd import checkpoint as ck

    class Ema:                                                      # torch_ema's interface: state_dict / load_state_dict
        def __init__(self, v):
            self.v = v

        def state_dict(self):
            return {'decay': 0.95, 'shadow_params': [self.v.clone()]}

        def load_state_dict(self, sd):
            self.v = sd['shadow_params'][0].clone()

    m = _model()
    opt = torch.optim.Adam(m.get_params(1e-3), betas=(0.9, 0.99), eps=1e-15)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 0.1 ** min(it / 100, 1))          # main.py:189
    for _ in range(5):
        opt.step(); sched.step()
    ema = Ema(torch.arange(4.0))
    path = ck.save_checkpoint(str(tmp_path / "df_ep0001.pth"), m, epoch=1, global_step=5, optimizer=opt, full=True, lr_scheduler=sched, ema=ema)
    raw = torch.load(path, weights_only=False)
    assert {'optimizer', 'lr_scheduler', 'ema'} <= set(raw) and 'scaler' not in raw
    m2 = _model()
    opt2 = torch.optim.Adam(m2.get_params(1e-3), betas=(0.9, 0.99), eps=1e-15)
    sched2 = torch.optim.lr_scheduler.LambdaLR(opt2, lambda it: 0.1 ** min(it / 100, 1))
    ema2 = Ema(torch.zeros(4))
    ck.load_checkpoint(m2, path, optimizer=opt2, lr_scheduler=sched2, ema=ema2)
    assert sched2.last_epoch == sched.last_epoch == 5 and torch.equal(ema2.v, torch.arange(4.0))


def test_half_table_invalidation_hooks():
    """`.data` writes do not move the version counter the fp16 shadow is keyed on: reset_parameters() and load_checkpoint() invalidate it"""
    from customnerf_amd import checkpoint as ck
    m = _model()
    enc = m.pos_en
    enc._half_version = ("stale",)
    enc.reset_parameters()
    assert enc._half_version is None
    enc._half_version = ("stale",)
    ck.load_checkpoint(m, {'model': m.state_dict()}, model_only=True, log=lambda *_: None)
    assert enc._half_version is None


# ------------------------------------------------------------------------------------------------ the reference's own file, as a fixture
def _reference_checkpoint():
    """tests/golden/checkpoint.{json,npz} (make_golden.py): the dict the reference's Trainer_Nerf.save_checkpoint(full=True) wrote for a tiny module
    with the reference's state-dict keys (cuda_ray), a two-group torch.optim.Adam after three applied steps and a skipped one, a LambdaLR and a
    GradScaler — rebuilt from the recorded structure, leaf types and arrays"""
    import collections
    import json
    import os
    import numpy as np
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "checkpoint.json")) as f:
        meta = json.load(f)
    arrays = np.load(os.path.join(here, "checkpoint.npz"))

    def build(n):
        t = n["t"]
        if t in ("dict", "OrderedDict"):
            return (dict if t == "dict" else collections.OrderedDict)((k, build(v)) for k, v in n["items"])
        if t in ("list", "tuple"):
            return (list if t == "list" else tuple)(build(v) for v in n["items"])
        if t == "Tensor":
            x = torch.from_numpy(np.array(arrays[n["a"]]))
            assert str(x.dtype) == n["dtype"]
            return x
        return n["v"]
    return build(meta["tree"]), meta


def _structure(x):
    """the nested key structure with the Python type (tensors: dtype and rank too) of every leaf"""
    if isinstance(x, dict):
        return (type(x).__name__, {k: _structure(v) for k, v in x.items()})
    if isinstance(x, (list, tuple)):
        return (type(x).__name__, [_structure(v) for v in x])
    if isinstance(x, torch.Tensor):
        return ("Tensor", str(x.dtype), x.dim())
    return type(x).__name__


class _Leafy(torch.nn.Module):
    def __init__(self, **named):
        super().__init__()
        for k, v in named.items():
            (self.register_parameter if isinstance(v, torch.nn.Parameter) else self.register_buffer)(k, v)


def _tiny_like(ref_model_sd, seed):
    """a module with the fixture's state-dict keys, shapes and dtypes and values of its own"""
    g = torch.Generator().manual_seed(seed)
    m = torch.nn.Module()
    subs = {}
    for k, v in ref_model_sd.items():
        fresh = torch.rand(v.shape, generator=g) if v.is_floating_point() else torch.randint(0, 50, v.shape, generator=g).to(v.dtype)
        if k.endswith((".embeddings", ".params")):
            fresh = torch.nn.Parameter(fresh - 0.5)
        if "." in k:
            subs.setdefault(k.split(".")[0], {})[k.split(".")[1]] = fresh
        else:
            m.register_buffer(k, fresh)
    for k in ("pos_en", "network", "density_network", "rgb_network"):     # registration order = parameter order = the optimiser's indices
        setattr(m, k, _Leafy(**subs[k]))
    m.cuda_ray, m.mean_count, m.mean_density = True, 0, 0.0
    return m


def _groups(m, lr=1e-3):
    return [{'params': [m.pos_en.embeddings], 'lr': lr * 10}, {'params': [m.network.params, m.density_network.params, m.rgb_network.params], 'lr': lr}]


def test_reference_written_checkpoint_structure_and_restore():
    """(1) checkpoint.checkpoint_state on equivalent objects has the reference file's keys and leaf types at every level; with this package's
    FusedAdam and DynamicLossScaler the only differences are the documented ones (Adam's 'step' an int, not a 0-dim tensor; torch.optim.Adam's
    remaining group defaults, which it fills in itself on load; the scaler's extra '_good_steps').  (2) checkpoint.load_checkpoint restores every entry of the
    reference-written dict.  (3) every key the reference's load_checkpoint reads (utils_init_nerf.py:847-901, recorded while it ran) is in a
    dict this package writes."""
    from customnerf_amd import checkpoint as ck
    from customnerf_amd.optim import DynamicLossScaler, FusedAdam
    ref, meta = _reference_checkpoint()
    assert meta["reference_loaded_this_packages_file"] is True
    lam = lambda it: 0.1 ** min(it / 100, 1)

    # (1) torch objects, as the reference's trainer holds them
    m = _tiny_like(ref['model'], 1)
    m.mean_count, m.mean_density = 12, 0.5
    opt = torch.optim.Adam(_groups(m), betas=(0.9, 0.99), eps=1e-15)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0, growth_interval=2)
    for _ in range(3):
        opt.zero_grad()
        scaler.scale(sum(p.sum() for p in m.parameters())).backward()
        scaler.step(opt); scaler.update(); sched.step()
    stats = {"loss": [0.25, 0.5], "valid_loss": [], "results": [], "checkpoints": ["x.pth"], "best_result": None}
    ours = ck.checkpoint_state(m, epoch=1, global_step=3, stats=stats, optimizer=opt, full=True, scaler=scaler, lr_scheduler=sched)
    assert list(ours) != [] and set(ours) == set(ref)
    assert _structure(ours) == _structure(ref)
    assert [tuple(v.shape) for v in ours['model'].values()] == [tuple(v.shape) for v in ref['model'].values()]
    # ... and this package's optimiser and scaler (state as after three applied steps and a skipped one: the host counter says 4, the device 3)
    fopt = FusedAdam(_groups(m), betas=(0.9, 0.99), eps=1e-15)
    for p in m.parameters():
        fopt.state[p] = {'step': 4, 'exp_avg': torch.zeros_like(p), 'exp_avg_sq': torch.zeros_like(p)}
    fsc = DynamicLossScaler("cpu", init_scale=1024.0, growth_interval=2)
    fsc.state[3] = 3.0
    fopt.scaler = fsc
    fsched = torch.optim.lr_scheduler.LambdaLR(fopt, lam)
    mine = ck.checkpoint_state(m, epoch=1, global_step=3, stats=stats, optimizer=fopt, full=True, scaler=fsc, lr_scheduler=fsched)
    s_mine, s_ref = _structure(mine), _structure(ref)
    assert set(mine) == set(ref)
    for k in ref:
        if k not in ('optimizer', 'scaler', 'lr_scheduler'):
            assert s_mine[1][k] == s_ref[1][k], k
    assert set(s_mine[1]['scaler'][1]) - set(s_ref[1]['scaler'][1]) == {'_good_steps'}
    assert all(s_mine[1]['scaler'][1][k] == v for k, v in s_ref[1]['scaler'][1].items())
    o_mine, o_ref = s_mine[1]['optimizer'][1], s_ref[1]['optimizer'][1]
    assert set(o_mine) == set(o_ref) and set(o_mine['state'][1]) == set(o_ref['state'][1]) == {0, 1, 2, 3}
    for i in range(4):
        assert o_mine['state'][1][i][1] == dict(o_ref['state'][1][i][1], step='int')
        assert mine['optimizer']['state'][i]['step'] == 3                          # the applied steps, not the calls of step()
    for gm, gr in zip(o_mine['param_groups'][1], o_ref['param_groups'][1]):
        assert set(gm[1]) <= set(gr[1]) and all(gr[1][k] == v for k, v in gm[1].items())
        # what torch.optim.Adam reads from a loaded group without a default of its own (Adam.__setstate__ fills in the rest)
        assert {'lr', 'betas', 'eps', 'weight_decay', 'amsgrad', 'params', 'initial_lr'} <= set(gm[1])

    # (2) every entry of the reference-written dict is restored
    m2 = _tiny_like(ref['model'], 2)
    opt2 = torch.optim.Adam(_groups(m2), betas=(0.9, 0.99), eps=1e-15)
    sched2 = torch.optim.lr_scheduler.LambdaLR(opt2, lam)
    sc2 = torch.amp.GradScaler("cpu")
    info = ck.load_checkpoint(m2, ref, optimizer=opt2, lr_scheduler=sched2, scaler=sc2)
    assert info['epoch'] == ref['epoch'] == 3 and info['global_step'] == ref['global_step'] == 4 and info['stats'] == ref['stats']
    assert info['missing_keys'] == [] and info['unexpected_keys'] == []
    assert m2.mean_count == ref['mean_count'] == 37 and m2.mean_density == ref['mean_density']
    for k, v in m2.state_dict().items():
        assert torch.equal(v, ref['model'][k]) and v.dtype == ref['model'][k].dtype, k
    back = opt2.state_dict()
    for i, st in ref['optimizer']['state'].items():
        assert int(st['step']) == 3
        for kk in st:
            assert torch.equal(back['state'][i][kk], st[kk]), (i, kk)
    assert back['param_groups'] == ref['optimizer']['param_groups']
    assert sched2.state_dict() == ref['lr_scheduler'] and sc2.state_dict() == ref['scaler']
    # ... into this package's optimiser and scaler too: the scaler's count of applied steps, which the reference's entry does not have, is Adam's
    m3 = _tiny_like(ref['model'], 3)
    fopt3 = FusedAdam(_groups(m3), betas=(0.9, 0.99), eps=1e-15)
    fsc3 = DynamicLossScaler("cpu")
    fopt3.scaler = fsc3
    ck.load_checkpoint(m3, ref, optimizer=fopt3, scaler=fsc3)
    assert fsc3.state.tolist() == [ref['scaler']['scale'], float(ref['scaler']['_growth_tracker']), 0.0, 3.0]
    assert fsc3.growth_interval == 2
    for p, i in zip(m3.parameters(), range(4)):
        st = fopt3.state[p]
        assert type(st['step']) is int and st['step'] == 3
        assert torch.equal(st['exp_avg'], ref['optimizer']['state'][i]['exp_avg']) and torch.equal(st['exp_avg_sq'], ref['optimizer']['state'][i]['exp_avg_sq'])
    assert fopt3.state_dict()['state'][0]['step'] == 3

    # (3) what the reference's load_checkpoint reads
    assert set(meta["reference_load_reads"]) == {'epoch', 'global_step', 'lr_scheduler', 'mean_count', 'mean_density', 'model', 'optimizer', 'scaler', 'stats'}
    for wrote in (ours, mine):
        assert set(meta["reference_load_reads"]) <= set(wrote)
    plain = ck.checkpoint_state(m, epoch=1, global_step=3)                       # not `full`: what it reads without asking first
    assert {'model', 'stats', 'epoch', 'global_step'} <= set(plain)
    assert set(meta["reference_load_reads"]) - set(meta["reference_load_probes"]) <= set(plain)
    assert {"loss", "valid_loss", "results", "checkpoints", "best_result"} <= set(plain['stats'])      # utils_init_nerf.py:808-821 index these
